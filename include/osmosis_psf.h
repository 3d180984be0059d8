/* osmosis_psf.h -- point-spread-function operators (motion blur, a measured PSF: 2-D kernels that do not factor per axis) of
 * libosmosis_hip.so: the third header of the library's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a
 * negative osm_status on failure with osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t,
 * NULL = default stream) and osmosis_linop.h.  Strict C99.
 *
 * A PSF travels as a tap list on the device: dy[T], dx[T] (int offsets from the anchor) and w[T] (fp32).  With
 *
 *   refl_n(c) = -c             if c < 0
 *             = 2 (n - 1) - c  if c >= n
 *             = c              otherwise                    (torch 'reflect' padding: no edge repeat)
 *
 * the forward map (adjoint = 0) is reflection padding followed by cross-correlation, as nn.Conv2d does it: for b < B, p < P
 *
 *   out[b,p,i,j] = sum_t w[t] * x[b,p, refl_H(i + dy[t]), refl_W(j + dx[t])]
 *
 * and adjoint = 1 is the exact transpose of that map in gather form,
 *
 *   g[b,p,r,s] = sum_t w[t] * sum_{i in pre_H(r,dy[t])} sum_{j in pre_W(s,dx[t])} v[b,p,i,j]
 *
 * pre_n(r, d) = the rows i in [0,n) with refl_n(i + d) = r:  i = r - d (direct),  i = -r - d only when r >= 1 (low mirror),
 * i = 2 (n - 1) - r - d only when r <= n - 2 (high mirror), each kept only where it lands in [0,n).  On a small image both
 * mirrors can hit the same pixel; both count.
 *
 * Elements: x[b * x_img_stride + p * H * W + i * W + j], out alike with out_img_stride; input and output share the H x W
 * grid.  The `zero_planes` planes that follow plane P - 1 of every output image are written as +0, so the call can read the
 * colour planes of a [B,C,HW] tensor and write those of another, depth plane included.
 *
 * Ry, Rx: the largest |dy| and |dx| of the list, stated by the caller (0 <= Ry < H, 0 <= Rx < W: reflection needs it); they
 * size the halo a workgroup stages.  A tap with |dy| > Ry or |dx| > Rx is skipped, never read.
 *
 * Summation order (fixed; every output element is written by exactly one lane, no atomics -- the bits depend on neither B
 * nor the launch shape nor on whether a tile was staged through LDS):
 *   forward:  acc = +0; for t = 0 .. T-1 ascending: acc = fma(w[t], x[..], acc).
 *   adjoint:  with vz = v extended by zeros outside [0,H) x [0,W) and
 *               G(c, e) = (acc = +0; for t ascending: acc = fma(w[t], vz[c - dy[t], e - dx[t]], acc)),
 *             rho_0(r) = r,  rho_1(r) = -r (r >= 1),  rho_2(r) = 2 (H - 1) - r (r <= H - 2), sigma_0..2(s) alike with W:
 *               g[r,s] = G(rho_0 r, sigma_0 s); then for (a, b) = (0,1), (0,2), (1,0), (1,1), ... (2,2) in this order, where
 *               both rho_a(r) and sigma_b(s) exist:  g[r,s] = g[r,s] + G(rho_a r, sigma_b s).
 *             (The inner sums of the formula above, regrouped by mirror: the same terms, each tap one fma.) */
#ifndef OSMOSIS_PSF_H
#define OSMOSIS_PSF_H

#ifdef __cplusplus
extern "C" {
#endif

int osm_psf_apply(const float* x, float* out,
                  const int* dy, const int* dx, const float* w, int T,   /* [T] each */
                  int Ry, int Rx,
                  int B, int P, long long x_img_stride, long long out_img_stride,
                  int H, int W,
                  int adjoint, int zero_planes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_PSF_H */
