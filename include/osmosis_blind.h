/* osmosis_blind.h -- blind deblurring: learning the weights of a point-spread function on the device, the sixth header of
 * libosmosis_hip.so's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with
 * osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream) and
 * osmosis_psf.h (the tap list dy[T], dx[T], w[T], refl_n and the forward / adjoint maps A(w), A(w)^T are the ones defined there).
 * Strict C99.
 *
 * The data term of the rgb-guidance ('ps') branch through a PSF whose weights are unknown: with rho_b = M_b (y_b - A(w) x0_b[0:3]),
 * loss_b = ||rho_b||_2 and r_b = d loss_b / d (A x0_b) (what osm_ps_loss_grad_c / _mc write), the weights descend the squared,
 * size-normalised objective
 *
 *   Q(w) = sum_b ||rho_b||^2 / (2 * 3 h w),     dQ/dw[t] = (1 / (3 h w)) sum_b loss_b c_b[t],
 *   c_b[t] = sum_{p < P} sum_{i, j} r_b[p,i,j] * x0_b[p, refl_H(i + dy[t]), refl_W(j + dx[t])]
 *
 * (c: the correlation of the residual's gradient with the image; the identity <r, A(w) x> = sum_t w[t] c[t] holds), one PSF
 * for the whole batch, kept on the simplex {w >= 0, sum w = 1} by a projected step.
 *
 * osm_psf_tap_grad -- the partial sums of c.  Gather form, no atomics: every element of `part` is written by exactly one lane.
 *   A workgroup owns one 32 x 32 tile (ragged at the image's far edges) of one plane p of one image b; tiles are numbered
 *   q = p * ntiles + ty * ntx + tx with ntx = ceil(W / 32), nty = ceil(H / 32), ntiles = ntx * nty.  Summation order (fixed):
 *     part[b][q][t] = (acc = +0; for i ascending over the tile's rows, for j ascending over its columns:
 *                      acc = fma(r[b,p,i,j], x[b,p,refl_H(i + dy[t]), refl_W(j + dx[t])], acc))           -- fp32, one fma per pixel
 *   so the longest fp32 chain is the 1024 pixels of a full tile, and the bits depend on neither B nor the launch shape.
 *   c_b[t] = sum over q ascending of (double)part[b][q][t] is formed in fp64 by osm_psf_tap_step (or by the caller).
 *   A tap with |dy[t]| > Ry or |dx[t]| > Rx is skipped, never read: its partials are written as +0.  The list need not be dense.
 *   Elements: x[b * x_img_stride + p * H * W + i * W + j], r alike with r_img_stride; part: [B][P * ntiles][T] floats, every one
 *   written.  0 <= Ry, Rx <= 32 (the window a workgroup stages: k <= 65 per side), Ry < H, Rx < W (reflection needs it).
 *
 * osm_psf_tap_step -- one projected step of w, ONE workgroup of 1024 lanes, all arithmetic fp64 in this order:
 *     c[b][t] = (s = 0; for q = 0 .. nparts-1 ascending: s += part[b][q][t])
 *     g[t]    = (s = 0; for b = 0 .. B-1 ascending: s += loss[b] * c[b][t]) / hw3                         (hw3 = 3 h w)
 *     gbar    = SUM_t(g) / T
 *     v[t]    = w[t] - eta * (g[t] - gbar) - eta * l1;      u[t] = v[t] > 0 ? v[t] : 0                    (a NaN v gives u = 0)
 *     S       = SUM_t(u)
 *     if S > 0 and S is finite:  w[t] = (float)(u[t] / S)   else w is left untouched
 *   SUM_t(a): lane l forms a_l = (s = 0; for t = l, l + 1024, ... ascending: s += a[t]); then for h = 512, 256, ... 1:
 *   a_l += a_{l + h} for l < h; the sum is a_0.  Subtracting gbar keeps the step in the plane sum w = 1 (clamping and
 *   renormalising alone has a biased fixed point); a non-finite loss or gradient leaves the estimate as it was.
 *   1 <= T <= OSM_BLIND_MAX_TAPS.
 *
 * osm_ps_blind_optimize -- one guided sub-step, enqueued by one call, no host synchronisation.  For i = 0 .. n_iter-1:
 *     Ax = A(w_i) x0[:, 0:3]                         osm_psf_apply (P = 3, image stride C H W)
 *     (loss_i, r_i)                                  osm_ps_loss_grad_c, or _mc with `mask` ([B,3,HW] rows; NULL: unmasked)
 *     tpart = tap partials of (r_i, x0)              osm_psf_tap_grad
 *     on the last iteration only: g[:, 0:3] = A(w_i)^T r_i, planes 3 .. C-1 written as +0      osm_psf_apply, adjoint
 *     w_{i+1} = step(w_i, tpart, loss_i)             osm_psf_tap_step
 *   5 n_iter + 1 launches; `loss` and `g` are those BEFORE the last step of w (as the Osmosis conditioner treats phi).  A fully
 *   masked image has loss = 0 and r = 0 and adds nothing to the step.  Everything is validated before the first launch.
 *   Workspaces: Ax, r [B][3][HW]; lpart [B * osm_phys_nblk(HW)]; tpart [B][3 * ntiles][T]. */
#ifndef OSMOSIS_BLIND_H
#define OSMOSIS_BLIND_H

#ifdef __cplusplus
extern "C" {
#endif

#define OSM_BLIND_MAX_TAPS 4225   /* (2 * 32 + 1)^2 */

int osm_psf_tap_grad(const float* x, const float* r,
                     const int* dy, const int* dx, int T,   /* [T] each */
                     int Ry, int Rx,
                     int B, int P, long long x_img_stride, long long r_img_stride,
                     int H, int W,
                     float* part, void* stream);

int osm_psf_tap_step(float* w, const float* part, const float* loss,
                     int B, int nparts, int T, long long hw3, double eta, double l1, void* stream);

int osm_ps_blind_optimize(const float* x0, const float* y, const float* mask /* NULL ok */,
                          const int* dy, const int* dx, float* w, int T, int Ry, int Rx,
                          int B, int C, int H, int W,
                          float* Ax, float* r, float* lpart, float* tpart, float* loss, float* g,
                          int n_iter, double eta, double l1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_BLIND_H */
