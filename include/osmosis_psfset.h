/* osmosis_psfset.h -- point-spread functions per image and per colour plane: weight SETS for the PSF operator and for blind
 * deblurring, the eleventh header of libosmosis_hip.so's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a
 * negative osm_status on failure with osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t,
 * NULL = default stream), osmosis_psf.h (the tap list, refl_n, the forward / adjoint maps and their summation order) and
 * osmosis_blind.h (the tap gradient, the projected step and its SUM_t).  Strict C99.
 *
 * The tap list dy[T], dx[T] stays shared; the weights become w[nb][nc][T], fp32, contiguous, nb in {1, B} (one set per image, or
 * one for all) and nc in {1, P} (one set per colour plane, or one for all).  Plane p of image b uses set
 * (per_image ? b : 0, per_channel ? p : 0).
 *
 * osm_psf_apply_s -- osm_psf_apply with the weights of plane (b, p) at  w + b * w_img_stride + p * w_plane_stride  (elements).
 *   Strides are >= 0; a non-zero plane stride is >= T; a non-zero image stride covers an image's planes:
 *   w_img_stride >= (w_plane_stride ? (P - 1) * w_plane_stride : 0) + T.  w[nb][nc][T] contiguous has strides
 *   (nb > 1 ? nc * T : 0, nc > 1 ? T : 0).  Forward and adjoint maps, summation order, mirrors, `zero_planes` and the staged /
 *   unstaged paths are osmosis_psf.h's, word for word; it is the same kernel.  The set is uniform per workgroup (a workgroup owns a
 *   tile of one plane of one image).  Strides (0, 0) are bit-identical to osm_psf_apply, and any plane (b, p) is bit-identical to
 *   osm_psf_apply run on that plane alone with that set.
 *
 * osm_psf_tap_step_s -- one projected step PER SET: nb * nc workgroups of 1024 lanes, nb = per_image ? B : 1,
 *   nc = per_channel ? P : 1, set (bi, ci) at w + (bi * nc + ci) * T.  `part` is osm_psf_tap_grad's [B][P * ntiles][T] with
 *   q = p * ntiles + tile.  All arithmetic fp64, osm_psf_tap_step's order on the set's own images and partials:
 *     images    b = bi if per_image, else 0 .. B-1 ascending
 *     partials  q in [ci * ntiles, (ci + 1) * ntiles) if per_channel, else [0, P * ntiles), ascending
 *     c[b][t] = (s = 0; for q ascending: s += part[b][q][t])
 *     g[t]    = (s = 0; for b ascending: s += loss[b] * c[b][t]) / hw3          (the same hw3 = 3 h w for every set)
 *     gbar = SUM_t(g) / T;  v[t] = w[t] - eta * (g[t] - gbar) - eta * l1;  u[t] = v[t] > 0 ? v[t] : 0;  S = SUM_t(u)
 *     if S > 0 and S is finite:  w[t] = (float)(u[t] / S)   else this set is left untouched (the others step)
 *   Each set lives on its own simplex; SUM_t is osmosis_blind.h's.  Q = sum_b ||rho_b||^2 / (2 * 3 h w) is unchanged: each set
 *   descends its own block of it (the planes / images that read the set).  Flags (0, 0) are bit-identical to osm_psf_tap_step with
 *   nparts = P * ntiles; with per_image, set b is bit-identical to osm_psf_tap_step(w_b, part[b], loss + b, B = 1); with
 *   per_channel at B = 1, set c is bit-identical to osm_psf_tap_step on the slice part + c * ntiles * T with nparts = ntiles.
 *   osm_psf_tap_grad is untouched: it never reads w, and its partial layout already separates the planes.
 *   1 <= T <= OSM_BLIND_MAX_TAPS, nb * nc <= 65535.
 *
 * osm_ps_blind_optimize_s -- osm_ps_blind_optimize with the two flags (P = 3 colour planes: nc = per_channel ? 3 : 1,
 *   w[nb][nc][T]): the same 5 n_iter + 1 launches through osm_psf_apply_s and osm_psf_tap_step_s, everything validated before
 *   the first launch.  With per_image, a B = 2 call is bit-identical to two B = 1 calls of osm_ps_blind_optimize (w, loss, g);
 *   flags (0, 0) are bit-identical to osm_ps_blind_optimize.  Workspaces as there. */
#ifndef OSMOSIS_PSFSET_H
#define OSMOSIS_PSFSET_H

#ifdef __cplusplus
extern "C" {
#endif

int osm_psf_apply_s(const float* x, float* out,
                    const int* dy, const int* dx, const float* w, int T,   /* dy, dx [T]; w: the sets */
                    int Ry, int Rx,
                    int B, int P, long long x_img_stride, long long out_img_stride,
                    int H, int W,
                    int adjoint, int zero_planes,
                    long long w_img_stride, long long w_plane_stride, void* stream);

int osm_psf_tap_step_s(float* w, const float* part, const float* loss,
                       int B, int P, int ntiles, int T, long long hw3, double eta, double l1,
                       int per_image, int per_channel, void* stream);

int osm_ps_blind_optimize_s(const float* x0, const float* y, const float* mask /* NULL ok */,
                            const int* dy, const int* dx, float* w, int T, int Ry, int Rx,
                            int B, int C, int H, int W,
                            float* Ax, float* r, float* lpart, float* tpart, float* loss, float* g,
                            int n_iter, double eta, double l1, int per_image, int per_channel, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_PSFSET_H */
