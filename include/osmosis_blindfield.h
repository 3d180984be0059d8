/* osmosis_blindfield.h -- blind spatially varying deblurring: learning a FIELD of point-spread functions on the device.  The
 * thirteenth header of libosmosis_hip.so's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status
 * on failure -- OSM_ERR_INVALID for a bad argument: nothing was launched; OSM_ERR_LAUNCH for a failed launch or copy -- with
 * osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream),
 * osmosis_psffield.h (the field operator A(w), its nodes, tables and hats) and osmosis_blind.h (the objective, osm_psf_tap_grad and
 * osm_psf_tap_step).  Strict C99, no struct.
 *
 * The reference has no such operator; these definitions are the contract.
 *
 * Tap list  dy[T], dx[T] int offsets from the anchor, shared by the nodes;  refl_n(c) = -c if c < 0;  2 (n - 1) - c if c >= n;  c
 *           otherwise;  Ry, Rx: the largest |dy|, |dx|, stated by the caller, 0 <= Ry <= 32, Ry < H, Rx alike with W; a tap beyond
 *           them is never read.  1 <= T <= OSM_FIELD_MAX_TAPS.  Weights w[gh][gw][T] fp32 contiguous: one PSF per node.
 * Nodes     those of osmosis_psffield.h: node j of a row at x = j (W - 1) / (gw - 1), rows alike; 2 <= gh <= min(H, 32),
 *           2 <= gw <= min(W, 32).  Tables iy0[H] int32, fy[H] fp32, ix0[W] int32, fx[W] fp32: the cell index (non-decreasing; clamped
 *           into [0, gh - 2] / [0, gw - 2] wherever it is read) and the position inside the cell.
 * Hats      a = 1 - fx;  b = 1 - fy  (fp32, one rounding each);  hatx_jx(x) = a where ix0[x] = jx, fx where ix0[x] = jx - 1, and
 *           structurally ABSENT elsewhere;  haty_jy(y) alike;  hat_n(p) = fl(haty_jy(y) hatx_jx(x)) for node n = (jy, jx), ONE fp32
 *           product, present where both axis hats are (a present hat may have the value 0).
 *
 * The objective is that of osmosis_blind.h with the field operator A(w) of osmosis_psffield.h in the PSF's place:
 *     Q(w) = sum_b ||rho_b||^2 / (2 * 3 h w),   dQ/dw_n[t] = (1 / (3 h w)) sum_b loss_b c_n[b][t],
 *     c_n[b][t] = sum_{p < P} sum_{i, j} hat_n(i, j) r_b[p,i,j] x_b[p, refl_H(i + dy[t]), refl_W(j + dx[t])]
 * with loss_b and r_b as osm_ps_loss_grad_c / _mc write them;  sum_n sum_t w_n[t] c_n[b][t] = <r_b, A(w) x_b>.
 *
 * Tiles and layout.  The image is cut into 32 x 32 tiles (ragged at the far edges), ntx = ceil(W / 32), nty = ceil(H / 32).  Node
 * (jy, jx) REACHES tile (ty, tx) when some row i of the tile has iy0[i] in {jy - 1, jy} and some column j has ix0[j] in {jx - 1, jx}: a
 * test on the tables alone, not on the hat's value.  The tables are non-decreasing, so the tile rows a node reaches are an interval
 * [ty0[jy], ty1[jy]) and the tile columns an interval [tx0[jx], tx1[jx]).  osm_field_tap_layout (HOST only: it reads host copies of
 * iy0, ix0 and touches no device) fills the int array
 *     lay = ty0[gh], ty1[gh], tx0[gw], tx1[gw], off[gh gw + 1]                          (OSM_FIELD_LAY_INTS(gh, gw) ints)
 * with off[0] = 0, off[n + 1] = off[n] + P (ty1 - ty0)(tx1 - tx0) for n = jy gw + jx ascending, and returns the float count
 * B off[gh gw] T of `part` (< 0 on failure).  The partial of image b, node n, plane p, tile (ty, tx) is the T floats at
 *     part[((b NP + off[n] + (p nty_n + (ty - ty0[jy])) ntx_n + (tx - tx0[jx])) T],   NP = off[gh gw], nty_n = ty1 - ty0, ntx_n alike
 * (per image; per node; plane-major; the node's tiles row-major).  Elements outside do not exist; every element inside is written.
 * The two kernels take `lay` as a DEVICE copy of that array.
 *
 * osm_field_tap_grad -- the per-node partials of c.  Gather form, no atomics, every element written by exactly one lane.  A
 * workgroup owns one tile of one plane of one image.  For every node n that reaches the tile and every tap t:
 *     part(b, n, p, tile)[t] = (acc = +0; for i ascending, j ascending over the tile's pixels where hat_n is present:
 *                               acc = fma(fl(hat_n(i, j) r[b,p,i,j]), x[b,p, refl_H(i + dy[t]), refl_W(j + dx[t])], acc))
 * fp32, one fma per pixel, the longest chain the 1024 pixels of a full tile; the hat and its product with r are never contracted.
 * A tap beyond (Ry, Rx) is written as +0.  For finite x and r this is bit for bit what osm_psf_tap_grad writes for that tile when
 * handed q_n = fl(hat_n (.) r) (0 where absent) in r's place (an absent pixel adds a zero product there); the bits depend on
 * neither B nor the launch shape.  A (node, tile) pair outside `lay`'s ranges is not written (tables that are not non-decreasing).
 * Elements: x[b * x_img_stride + p * H * W + i * W + j], r alike.  P H W < 2^31, W <= 2^28, B P <= 65535, ceil(H / 32) <= 65535.
 * Error against float64 on the same fp32 inputs, first order, u = 2^-24, per partial of n pixels:  (n + 3) u sum hat_n |r| |x|
 * (a, b, the hat, the product with r, then the chain).
 *
 * osm_field_tap_step -- one projected step of EVERY node, one 1024-lane workgroup per node, all arithmetic fp64 in this order:
 *     c_n[b][t] = (s = 0; for q = 0 .. P nty_n ntx_n - 1 ascending (plane, then tile): s += part(b, n, q)[t])
 *     g_n[t]    = (s = 0; for b ascending: s += loss[b] * c_n[b][t]) / hw3
 *     s_n[t]    = (s = 0; for the EXISTING 4-neighbours m in the order up (jy - 1), left (jx - 1), right, down: s += (w_n[t] - w_m[t]))
 *     gbar      = SUM_t(g_n) / T
 *     v[t]      = ((w_n[t] - eta * (g_n[t] - gbar)) - eta * l1) - (eta * smooth) * s_n[t];    u[t] = v[t] > 0 ? v[t] : 0   (NaN: 0)
 *                 (the last term is left out altogether when smooth = 0)
 *     S         = SUM_t(u);   S > 0 and finite:  w_new_n[t] = (float)(u[t] / S)   else  w_new_n[t] = w_n[t]
 * SUM_t(a): lane l forms (s = 0; for t = l, l + 1024, ... ascending: s += a[t]); then for h = 512, 256, ... 1: a_l += a_{l + h} for
 * l < h; the sum is a_0 (osm_psf_tap_step's).  The kernel reads w and writes the workspace w_new ([gh][gw][T], never aliasing w: a
 * node reads its neighbours while they step); the entry point then copies w_new -> w on the same stream, so w stays the one live
 * tensor.  With smooth = 0 a node's step is bit for bit osm_psf_tap_step on that node's partials repacked as [B][nparts][T].
 * smooth >= 0 and finite; eta, l1 not NaN; hw3 = 3 h w >= 1.
 *
 * There is no "optimize" entry point: a guided sub-step is enqueued by the caller, launch by launch, stream-ordered:
 * osm_psf_field_apply; osm_ps_loss_grad_c / _mc; osm_field_tap_grad; on the last iteration only the adjoint
 * osm_psf_field_apply into g; osm_field_tap_step.
 *
 * Kernels (csrc/blindfield.hip, compiled without floating-point contraction): gfx950, wave64.  Tap gradient: 256-thread workgroups;
 * the reflected window of x and the tile of r are staged in LDS once; per reaching node the tile of q_n is formed in LDS and lanes
 * tid, tid + 256, ... walk it, one tap each. */
#ifndef OSMOSIS_BLINDFIELD_H
#define OSMOSIS_BLINDFIELD_H

#ifdef __cplusplus
extern "C" {
#endif

#define OSM_FIELD_MAX_TAPS 4225                               /* (2 * 32 + 1)^2 */
#define OSM_FIELD_LAY_INTS(gh, gw) (2 * (gh) + 2 * (gw) + (gh) * (gw) + 1)

/* HOST only.  iy0 [H], ix0 [W]: host arrays; lay: host, OSM_FIELD_LAY_INTS(gh, gw) ints.  Returns the float count of `part`, < 0 on failure */
long long osm_field_tap_layout(int gh, int gw, const int* iy0, const int* ix0,
                               int H, int W, int P, int B, int T, int* lay);

int osm_field_tap_grad(const float* x, const float* r,
                       const int* dy, const int* dx, int T,   /* [T] each */
                       int Ry, int Rx,
                       int gh, int gw, const int* iy0, const float* fy, const int* ix0, const float* fx,
                       const int* lay,                        /* device copy of the layout */
                       int B, int P, long long x_img_stride, long long r_img_stride,
                       int H, int W,
                       float* part, void* stream);

int osm_field_tap_step(float* w, float* w_new, const float* part, const float* loss,
                       const int* lay, int gh, int gw,
                       int B, int T, long long hw3, double eta, double l1, double smooth, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_BLINDFIELD_H */
