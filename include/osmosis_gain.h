/* osmosis_gain.h -- a learnt vignetting gain field in the Osmosis data term, the tenth header of libosmosis_hip.so's C ABI, beside
 * osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with osm_last_error() naming it, device
 * pointers owned by the caller, `stream` a hipStream_t, NULL = default stream) and osmosis_physlin.h (F is osm_phys_forward's).
 * Strict C99.
 *
 * The reference has no such term; these definitions are the contract.
 *
 * The photo is modelled as y01 = G F(x0; phi): F the model image, G > 0 one smooth gain per pixel, the same for the three channels
 * (lens vignetting, the fall-off of a strobe).  With y = 2 y01 - 1 the residual of the model G F,
 *     r_c = (y_c - (2 G F_c - 1)) w M_c = ((y_c + 1) / G - 1 - (2 F_c - 1)) w (M_c G),
 * is the existing masked residual on y' = (y + 1) / G - 1 with the mask M' = M G: loss, phi step and dL/dx0 of the model G F are
 * those of osm_phys_optimize_m / _g called with (y', M').  This header makes (y', M') and learns G.
 *
 * Field    nodes n [B][gh][gw] fp32, 2 <= gh <= min(H, 32), 2 <= gw <= min(W, 32), on the image corners inclusive: node j of a row
 *          sits at x = j (W - 1) / (gw - 1) (rows alike with H, gh).  G = the bilinear interpolation of the nodes, from the tables
 *          iy0 [H] int32, fy [H] fp32, ix0 [W] int32, fx [W] fp32 (cell index in [0, gh - 2] / [0, gw - 2], non-decreasing, and the
 *          position inside the cell in [0, 1]; built on the host in float64 and rounded to fp32; the kernels clamp the indices):
 *              a = 1 - fx;  b = 1 - fy                                     (fp32, one rounding each: the hat weights everywhere)
 *              top = a n00 + fx n01;  bot = a n10 + fx n11;  G = b top + fy bot
 *          every product and every sum rounded once in fp32, in this order (never an fma); n00 = n[iy0][ix0], n01 = n[iy0][ix0 + 1],
 *          n10 = n[iy0 + 1][ix0], n11 = n[iy0 + 1][ix0 + 1].  hat_j(p) = haty_jy(y) hatx_jx(x), hatx_jx(x) = a where ix0[x] = jx,
 *          fx where ix0[x] = jx - 1, else 0.
 * Expand   y'_c = (y_c + 1) / G - 1 (a sum, an IEEE division, a difference; nothing fused); M'_c = M0_c G, M0 [B,3,HW], NULL = ones
 *          (M' = G); G itself is written as field [B,1,HW].
 * Gradient at the phi the sub-step starts from, on F [B,P,HW] (P = 4: plane 3 is the depth weight w; P = 3: w = 1), per pixel, fp32,
 *          each operation rounded once, left to right:
 *              r_c = ((y_c - (2 (G F_c) - 1)) w) M0_c;   d_c = ((-2 F_c) w) M0_c
 *              q = (r_0 d_0 + r_1 d_1) + r_2 d_2         (= sum_c r_c dr_c/dG)
 *          t[b][y][jx] = sum over the node's support, ascending x, of hatx_jx(x) q(y, x)    (fp32; the product rounded, then added)
 *          s[b][y]     = sum of r_c^2 over the row: lane l of 64 adds x = l, l + 64, ..., c = 0, 1, 2 inside a pixel, then the
 *                        xor tree 32, 16, 8, 4, 2, 1                                         (fp32)
 *          c_raw[jy][jx] = sum over ascending y of haty_jy(y) t[y][jx], S = sum over ascending y of s[y]      (float64)
 *          c = gscale c_raw, gscale = 1 / sqrt(S) (norm: L = sqrt(S)) or 2 / (3 HW) (mse: L = S / (3 HW)): c = dL / dn.
 * Step     one per image, float64, nodes read as fp32 and stored back rounded to fp32:
 *              u = max(n - eta (c + lambda Ln), g_min)     Ln = the gradient of 1/2 sum_edges (n_i - n_j)^2 on the 4-neighbour
 *                                                          node graph: sum of (n - n_k) over k = up, left, right, down
 *              n <- u / max(u)                             the gauge max n = 1: a global gain is a scaling of J and phi_inf
 *              n <- max(n, g_min)
 *          max(v, g_min) is v < g_min ? g_min : v, so a NaN survives into max(u).  Guards, each leaving the image's nodes
 *          untouched: S not finite; S = 0 under the norm loss (a fully masked image); max(u) not finite.
 *          g_min > 0, eta >= 0, lambda >= 0, all finite.
 * Sub-step n_iter (>= 1) x { gradient, step }, then one expand at the final nodes; freeze_phi or learn = 0: the expand alone.
 *
 * Error of t / s against float64 on the same fp32 inputs, first order with u = 2^-23 (twice the unit roundoff, which pays for the
 * second-order terms), G, F, r, d, q below the float64 values and e_c = y_c - (2 G F_c - 1):
 *     dr_c      = w M0_c (14 |G F_c| + |2 G F_c - 1| + 3 |e_c|)       (6 roundings in G, one in G F, doubled; then P, e, w, M0)
 *     |c_raw err| <= u sum_p hat_j(p) sum_c (|d_c| dr_c + (Kx + 8) |r_c d_c|)        Kx = the most pixels in a node's x support
 *     |S err|     <= u sum_p sum_c (2 |r_c| dr_c + (3 ceil(W / 64) + 7) r_c^2)
 * The float64 sums over y add nothing of this order.
 *
 * Kernels (csrc/gainfield.hip, compiled without floating-point contraction): wave64, 256-thread workgroups, gather form, no
 * floating-point atomics, no global atomics, fixed order: bit-reproducible, and the bits of an image do not depend on the batch.
 *
 * Shapes: F [B,P,HW]; y, M0, y_eff, m_eff [B,3,HW]; field [B,1,HW]; nodes [B,gh,gw]; t [B,H,gw]; s [B,H] fp32 contiguous;
 * cs [B][gh gw + 1] float64: c_raw then S of the last gradient.  H W < 2^29, B <= 65535; osm_gain_rows needs W <= 4096. */
#ifndef OSMOSIS_GAIN_H
#define OSMOSIS_GAIN_H

#include "osmosis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osm_gain_desc {
  int B;
  int H;
  int W;
  int gh;
  int gw;
  int P;          /* planes of F: 3, or 4 with the depth weight in plane 3 */
  int loss_type;  /* 0 norm, 1 mse */
  float eta;      /* step size, >= 0 */
  float lambda;   /* smoothness weight, >= 0 */
  float g_min;    /* floor of the nodes, > 0 */
  int n_iter;     /* gradient + step pairs per sub-step, >= 1 */
  int learn;      /* 0: the field is fixed (a measured flat field) */
} osm_gain_desc;

/* y_eff, m_eff and field from y, M0 (NULL: ones) and the nodes */
int osm_gain_expand(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx, const float* nodes,
                    const float* y, const float* M0, float* y_eff, float* m_eff, float* field, void* stream);

/* t and s of every pixel row from F, y, M0 (NULL: ones) and the nodes */
int osm_gain_rows(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx, const float* nodes,
                  const float* F, const float* y, const float* M0, float* t, float* s, void* stream);

/* cs = (c_raw, S) from t and s, then the step on the nodes in place */
int osm_gain_step(const osm_gain_desc* d, const int* iy0, const float* fy, const float* t, const float* s, float* nodes, double* cs,
                  void* stream);

/* the sub-step's 2 n_iter + 1 launches from one call (freeze_phi != 0 or learn = 0: the expand alone; F, t, s, cs may then be NULL) */
int osm_gain_prepare(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx, const float* F,
                     const float* y, const float* M0, float* nodes, float* t, float* s, double* cs, float* y_eff, float* m_eff,
                     float* field, int freeze_phi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_GAIN_H */
