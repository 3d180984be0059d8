/* osmosis_robust.h -- a robust data term: per-pixel IRLS weights from an on-device MAD scale, the ninth header of
 * libosmosis_hip.so's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with
 * osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream).  Strict C99.
 *
 * The reference has no such term; these definitions are the contract.
 *
 * Per guided sub-step and per image b, on the measurement's grid (hw pixels, three channels, entry i = c hw + p of 3 hw):
 *   prediction  P = pa pred + pb           pred: the first three planes of image b of a [B,*,hw] tensor, `pred_bstride` floats
 *                                          apart (the model image F[B,P,hw] of osm_phys_forward with (pa, pb) = (2, -1); x0[B,C,hw]
 *                                          of the identity term with (1, 0))
 *   residual    e = y - P                  UNFUSED, three fp32 operations of one rounding each: t = pa * pred; P = t + pb;
 *                                          e = y - P (never an fma).  Raw: no depth weight and no mask.
 *   valid       M0 > 0 and e finite        M0 [B,3,hw]: the base mask; a NULL M0 is a mask of ones.  n_b = the number of valid
 *                                          entries of image b, the three channels pooled.
 *   scale       mad:   a_lo, a_hi = the order statistics of rank (n_b - 1) >> 1 and n_b >> 1 (from 0, ascending) of |e| over the
 *                      valid entries; med = 0.5f * (a_lo + a_hi); sigma_b = max(1.4826f * med, sigma_min), every operation one fp32
 *                      rounding.  n_b = 0: sigma_b = NaN (and every entry is invalid).
 *               fixed: sigma_b = `scale` for every image; nothing is selected, sigma[] and n_valid[] are not touched by
 *                      osm_robust_mask.
 *   u           |e| / (c sigma_b)          cs = c * sigma_b, u = |e| / cs (IEEE division), and u = 0 where |e| = 0 (so that
 *                                          sigma_b = 0, possible with sigma_min = 0, keeps a zero residual an inlier).
 *                                          per_pixel: u of every valid channel of a pixel = the maximum over its valid channels.
 *   weight      loss 0 huber:  omega = u <= 1 ? 1 : 1 / u           sqrt(omega) = sqrtf(omega)
 *               loss 1 tukey:  omega = u < 1 ? (1 - u^2)^2 : 0      sqrt(omega) = 1 - u^2: no square root is taken
 *               loss 2 cauchy: omega = 1 / (1 + u^2)                sqrt(omega) = sqrtf(omega)
 *   mask        M_eff = M0 * sqrt(omega) on a valid entry; M_eff = M0 and omega = 1 on an entry that is not valid (M0 <= 0 gives
 *               0 or M0 itself, a non-finite e leaves M0 so that a NaN travels through the data term as it does without the term).
 *
 * The data term is the masked route (osm_phys_*_m, osm_ps_loss_grad_mc) with M_eff in M0's place; omega is a constant of the
 * sub-step (iteratively re-weighted least squares), nothing is differentiated through it.
 *
 * Kernels (csrc/robust.hip): wave64, no global atomics, fixed order: bit-reproducible, and the bits of an image do not depend on the
 * batch around it.  The select is exact: three radix passes over the 31-bit keys bits(e) & 0x7fffffff (11 / 10 / 10 bits) by one
 * 1024-lane workgroup per image, histograms in LDS with integer atomics, both ranks followed at once.  No workspace is needed.
 *
 * Shapes: e, M0, M_eff, omega [B,3,hw] fp32 contiguous; sigma [B] fp32; n_valid [B] int32. */
#ifndef OSMOSIS_ROBUST_H
#define OSMOSIS_ROBUST_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osm_robust_desc {
  int loss;         /* 0 huber, 1 tukey, 2 cauchy */
  float c;          /* tuning constant, > 0 */
  int scale_mode;   /* 0 mad, 1 fixed */
  float scale;      /* the fixed sigma, > 0 (read when scale_mode = 1) */
  float sigma_min;  /* >= 0 (mad) */
  int per_pixel;    /* 0 / 1 */
  int B;
  int hw;
} osm_robust_desc;

/* e[B,3,hw] = y - (pa pred + pb); pred_bstride >= 3 hw */
int osm_robust_resid(const osm_robust_desc* d, const float* pred, long long pred_bstride, float pa, float pb, const float* y, float* e,
                     void* stream);

/* the mad scale and n_b of every image (runs the select whatever scale_mode says) */
int osm_robust_scale(const osm_robust_desc* d, const float* e, const float* M0, float* sigma, int* n_valid, void* stream);

/* M_eff (and omega, when not NULL) from e, M0 and sigma[] (scale_mode 0) or `scale` (scale_mode 1: sigma may be NULL) */
int osm_robust_weights(const osm_robust_desc* d, const float* e, const float* M0, const float* sigma, float* M_eff, float* omega,
                       void* stream);

/* the launches from one call: resid, scale (scale_mode 0 only), weights */
int osm_robust_mask(const osm_robust_desc* d, const float* pred, long long pred_bstride, float pa, float pb, const float* y,
                    const float* M0, float* e, float* sigma, int* n_valid, float* M_eff, float* omega, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_ROBUST_H */
