/* osmosis_solver.h -- few-step solvers for the sampler step (DDIM, DPM-Solver++ 2M), the eighth header of libosmosis_hip.so's C ABI,
 * beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with osm_last_error() naming it,
 * device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream).  Strict C99.
 *
 * The step.  All tensors fp32 [B,C,HW]; per element e of channel c:
 *   t      = A x
 *   t     += B0 x0
 *   t     += B1 hist           only when B1 != 0: hist is not read otherwise and may hold anything
 *   t     += S z               only when S != 0, the row's noise_on != 0 and there is noise (a tensor, or the in-kernel draw)
 *   grad   = c0 g + dx_unet    one fused multiply-add, as osm_guide_update forms it; 0 and no subtraction when g is NULL
 *   x_next = t - scale[c] clamp(grad, -clip, clip)         clip < 0: no clamp; a NaN grad stays NaN (torch.clamp)
 *   hist   = x0                the same launch: the next index's history
 * Every product and every sum above is rounded once, in this order (no contraction).  x_next may alias x; hist is a buffer of
 * its own.  grad_out (grad) and noise_out (the z used, 0 where none was added) are optional.
 *
 * Rows, fetched by osm_fetch_coefs like every row:
 *   coef = the posterior row (osmosis_hip.h): only c0 = coef[0], d x0 / d x of the mean processor, is read
 *   srow = { A, B0, B1, S, noise_on, 0, 0, t_model }
 *
 * The rules the host puts into srow (float64, cast once).  At loop index i: ab = alphas_cumprod[i], ab' = alphas_cumprod_prev[i],
 * alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma), primes likewise; x0 is the processed pred_xstart.
 *   ddim, eta >= 0 (Song et al. 2021, eq. 12, in (x_t, x0) form):
 *     s = eta sqrt((1 - ab') / (1 - ab)) sqrt(1 - ab / ab'),  A = sqrt(1 - ab' - s^2) / sigma,  B0 = alpha' - A alpha,  B1 = 0,  S = s
 *   dpmpp_2m (Lu et al. 2022, DPM-Solver++ multistep, data prediction; deterministic):
 *     h = lambda' - lambda,  A = sigma' / sigma,  beta = -alpha' expm1(-h),  r = h_prev / h,
 *     B0 = beta (1 + 1 / (2 r)),  B1 = -beta / (2 r),  S = 0;   with no history (the first executed index): B0 = beta, B1 = 0,
 *     which is the ddim step at eta = 0
 *   the last index (ab' = 1), both rules: A = 0, B0 = 1, B1 = 0, S = 0 -- the sample is x0.
 *
 * A lane owns four consecutive elements: one 16-byte access per tensor when HW % 4 == 0 and every pointer is 16-byte aligned,
 * element by element otherwise (same values either way).
 *
 * osm_solver_update_rng_c draws z in the kernel: Philox-4x32-10 keyed by `seed`, counter (element quad of the image's C HW
 * elements, img0 + b img_stride, (*step + step_offset) | sub << 16, the step-noise stream) -- the words of osm_guide_update_rng_c,
 * so osm_randn_sub with n = C HW draws the same z.  It needs HW % 4 == 0 and 16-byte aligned tensors.
 *
 * Refused before any launch (OSM_ERR_INVALID): a NULL x0 / x / hist / coef / srow / x_next; B, C or HW < 1; g without scale; dx_unet
 * without g; a NaN clip; hist aliasing x0, x or x_next; for the rng form a NULL step, sub outside [0, 65536), HW % 4 != 0 or a
 * misaligned tensor. */
#ifndef OSMOSIS_SOLVER_H
#define OSMOSIS_SOLVER_H

#ifdef __cplusplus
extern "C" {
#endif

int osm_solver_update_c(const float* x0, const float* x, float* hist, const float* g, const float* dx_unet, const float* noise,
                        const float* coef, const float* srow, const float* scale, float clip, float* x_next, float* grad_out,
                        float* noise_out, int B, int C, int HW, void* stream);

int osm_solver_update_rng_c(const float* x0, const float* x, float* hist, const float* g, const float* dx_unet, const float* coef,
                            const float* srow, const float* scale, float clip, float* x_next, float* grad_out, float* noise_out,
                            int B, int C, int HW, unsigned long long seed, const int* step, int step_offset, int sub, int img0,
                            int img_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_SOLVER_H */
