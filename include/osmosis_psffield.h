/* osmosis_psffield.h -- spatially varying blur: a FIELD of point-spread functions on a coarse node grid, interpolated bilinearly over
 * the frame.  The twelfth header of libosmosis_hip.so's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a
 * negative osm_status on failure -- OSM_ERR_INVALID for a bad argument: nothing was launched; OSM_ERR_LAUNCH for a failed launch --
 * with osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream),
 * osmosis_psf.h (the tap list, refl_n, the forward / adjoint maps) and osmosis_gain.h (the node grid).  Strict C99, no struct.
 *
 * The reference has no such operator; these definitions are the contract.
 *
 * Tap list  dy[T], dx[T] int offsets from the anchor, SHARED by the nodes, as in osmosis_psf.h, with its
 *               refl_n(c) = -c if c < 0;  2 (n - 1) - c if c >= n;  c otherwise            (torch 'reflect' padding)
 *           and its Ry, Rx: the largest |dy|, |dx|, stated by the caller, 0 <= Ry < H, 0 <= Rx < W; a tap beyond them is skipped,
 *           never read.  Weights w[gh][gw][T] fp32 contiguous: one PSF per node (a node without a tap of the list carries 0).
 * Nodes     where the gain field's are (osmosis_gain.h): node j of a row at x = j (W - 1) / (gw - 1), rows alike with H, gh;
 *           2 <= gh <= min(H, 32), 2 <= gw <= min(W, 32).  Tables iy0[H] int32, fy[H] fp32, ix0[W] int32, fx[W] fp32: the cell index
 *           (in [0, gh - 2] / [0, gw - 2], non-decreasing; the kernel clamps it) and the position inside the cell in [0, 1], built on
 *           the host in float64 and rounded to fp32.
 * Hats      a = 1 - fx;  b = 1 - fy   (fp32, one rounding each);  hatx_jx(x) = a where ix0[x] = jx, fx where ix0[x] = jx - 1, else 0;
 *           haty_jy(y) alike;  hat_n(p) = haty_jy(y) hatx_jx(x) for node n = (jy, jx), ONE fp32 product.
 *
 * Forward (adjoint = 0): the blur with the interpolated kernel sum_n hat_n(p) K_n at every pixel p.  For pixel (i, j) of plane
 * (b, p < P), in cell (cy, cx) = (iy0[i], ix0[j]), and k, l in {0, 1}:
 *     c_kl = (acc = +0; for t = 0 .. T-1 ascending: acc = fma(w[cy + k][cx + l][t], x[b,p, refl_H(i + dy[t]), refl_W(j + dx[t])], acc))
 *     top = a c_00 + fx c_01;   bot = a c_10 + fx c_11;   out[b,p,i,j] = b top + fy bot
 * every product and every sum of the last line rounded once in fp32, in this order, never an fma (the G of osmosis_gain.h).  Every
 * c_kl is, by construction, bit for bit what osm_psf_apply writes at (i, j) with that node's weights.
 *
 * Adjoint (adjoint = 1): the exact transpose, in gather form.  With A_n = the adjoint map of osmosis_psf.h (all its mirror passes,
 * in its order, each tap one fma) for the weights of node n, applied to the plane u_n = fl(hat_n (.) v) (one fp32 product per pixel):
 *     g = (s = A_first; for the other nodes in ascending row-major order: s = s + A_n)
 * A node whose hat is zero on every source pixel that an output's passes read may be left out (it would add +0), so the result is
 * specified up to the sign of a zero, for finite w and v.
 *
 * Elements, image strides, P, `zero_planes` (written as +0), B and the limits on H, W are osm_psf_apply's:
 *     x[b * x_img_stride + p * H * W + i * W + j], out alike with out_img_stride;  (P + zero_planes) H W < 2^31;  W <= 2^28;
 *     B (P + zero_planes) <= 65535;  ceil(H / 32) <= 65535.
 * Everything is validated before the launch: null pointers, the grid limits, T >= 1, adjoint in {0, 1}, the radii, the strides.
 * One launch; no atomics; every output element is written by exactly one lane, with vector stores; the bits depend on neither B nor
 * the launch shape nor on whether a workgroup staged its window in LDS.
 *
 * Error against float64 on the same fp32 inputs (w, x or v, fy, fx; a and b exact there), first order, u = 2^-24:
 *     forward   |out - out64| <= (T + 8) u  sum_n hat_n(p) sum_t |w_n[t]| |x[refl(p + d_t)]|
 *               (each c_kl within (T + 2) u sum |w||x|, the bound of one convolution; on a corner's way to `out` six more roundings:
 *                a, a c, top, b, b top, out)
 *     adjoint   |g - g64|     <= (T + 14 + gh gw) u  sum_n (|A_n| (hat_n (.) |v|))        (|A_n|: A_n with the weights |w_n|)
 *               (four roundings in u_n -- a, b, the hat, the product with v --, (T + 2) u for a pass's taps, at most eight sums of
 *                passes and gh gw - 1 of nodes)
 * A field of identical nodes: |out - c| <= 8 u |c| with c = osm_psf_apply's value (six roundings of the combine, one each in a, b).
 *
 * Kernel (csrc/psffield.hip; the combine and the hats compiled without floating-point contraction): gfx950, wave64, 256-thread
 * workgroups, a 32 x 32 output tile per workgroup, a lane owns four consecutive outputs of a row; the window is staged in LDS
 * (once for the forward; per mirror pass and node for the adjoint), a window beyond the buffer is read from global memory in the
 * same order. */
#ifndef OSMOSIS_PSFFIELD_H
#define OSMOSIS_PSFFIELD_H

#ifdef __cplusplus
extern "C" {
#endif

int osm_psf_field_apply(const float* x, float* out,
                        const int* dy, const int* dx, const float* w, int T,   /* dy, dx [T]; w [gh][gw][T] */
                        int Ry, int Rx,
                        int gh, int gw, const int* iy0, const float* fy, const int* ix0, const float* fx,
                        int B, int P, long long x_img_stride, long long out_img_stride,
                        int H, int W,
                        int adjoint, int zero_planes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_PSFFIELD_H */
