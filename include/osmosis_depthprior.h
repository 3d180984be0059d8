/* osmosis_depthprior.h -- a range-map depth prior in the Osmosis data term, the seventh header of libosmosis_hip.so's C ABI, beside
 * osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with osm_last_error() naming it, device
 * pointers owned by the caller, `stream` a hipStream_t, NULL = default stream).  Strict C99.
 *
 * The reference has no such term; these definitions are the contract.
 *
 * Inputs, per image b and pixel p of the network grid (HW pixels):
 *   D  = x0[b,3,p]                         the network's depth plane (x0: [B,4,HW] fp32)
 *   d  = conv_depth(D; depth_type, dval)   the operator's own depth conversion (0 original: (D + 1) / 2; 1 gamma:
 *                                          ((D + v0) v1)^v2; 2 move: D + v0 -- osm_phys_desc's codes), the quantity inside the
 *                                          exponents of the image-formation model, so the prior constrains what phi multiplies
 *   dd = d d / d D
 *   z >= 0                                 the range prior [B,1,HW] fp32, any unit
 *   m in [0, 1]                            its confidence [B,1,HW] fp32, 0 where there is no range
 * A pixel with m = 0 (anything but m > 0) contributes exactly nothing, whatever z holds there: z is not used.
 *
 * Moments, fp64, over the pixels with m > 0, products formed in fp64 from the fp32 operands (mz = m z, md = m d):
 *   S_m = sum m,  S_z = sum mz,  S_d = sum md,  S_zz = sum mz z,  S_zd = sum mz d,  S_dd = sum md d
 * Summation order (fixed, no atomics: the bits depend on neither B nor the launch): workgroup k of image b owns the pixels
 * 1024 k .. 1024 k + 1023; its lane t adds p = 1024 k + t, + 256, + 512, + 768 ascending; the 64 lanes of a wave fold by
 * xor-butterfly 32, 16, .. 1; the four waves as (w0 + w1) + (w2 + w3) into part[b][k][0..5] (slots 6, 7 written as 0).
 * osm_depth_fit: component c's partials k = s, s + 4, ... (s = 0..3) ascending, then (s0 + s1) + (s2 + s3).
 *
 * Fit (a, c) per image, fp64:
 *   align 0 none:    a = scale, c = 0
 *   align 1 scale:   a = max(S_zd / S_zz, scale_min), c = 0
 *   align 2 affine:  det = S_m S_zz - S_z^2, a = max((S_m S_zd - S_z S_d) / det, scale_min), c = (S_d - a S_z) / S_m
 * scale_min > 0 keeps depth increasing with range.
 *
 * Loss and gradient:
 *   S = max(S_dd - 2 a S_zd - 2 c S_d + a^2 S_zz + 2 a c S_z + c^2 S_m, 0)
 *   loss_type 0 norm:  L = sqrt(S),  gs = lambda / L
 *   loss_type 1 mse:   L = S / S_m,  gs = 2 lambda / S_m        (S_m, not HW: a sparse map must not vanish)
 *   e = d - (a z + c) in fp64;  inc = (float)(gs m e dd);  g[b,3,p] = g[b,3,p] + inc in fp32     (g: [B,4,HW])
 * (a, c) are constants of the step: they minimise S (or a sits on its bound and c minimises), so by the envelope theorem this is the
 * exact gradient of lambda L.  g[:, 0:3] and the pixels with m = 0 are never written.  depth_loss[b] = (float)L, without lambda.
 *
 * Guards, per image.  A skipped image has L = 0, gs = 0 and g is not written for it; a, c are NaN unless align is none.
 *   S_m <= 0;  scale with S_zz <= 0;  affine with det <= 2^-40 S_m S_zz (a constant range map cannot fix two parameters);
 *   any moment non-finite: skipped, and L is reported as NaN;
 *   norm with S <= 2^-40 S_dd: a perfect fit, L = 0 and no gradient (torch.linalg.norm's backward at 0); a, c are kept.
 *
 * fit: double [B][4] = a, c, gs, L, on the device.  part: double [B][osm_depth_nblk(HW)][8]. */
#ifndef OSMOSIS_DEPTHPRIOR_H
#define OSMOSIS_DEPTHPRIOR_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osm_depth_desc {
  int align;      /* 0 none, 1 scale, 2 affine */
  int loss_type;  /* 0 norm, 1 mse */
  float lambda;
  float scale;
  float scale_min;
  int depth_type;
  float dval[3];
  int B;
  int HW;
} osm_depth_desc;

int osm_depth_nblk(int HW);

int osm_depth_reduce(const osm_depth_desc* d, const float* x0, const float* z, const float* m, double* part, void* stream);

int osm_depth_fit(const osm_depth_desc* d, const double* part, double* fit, float* depth_loss, void* stream);

int osm_depth_grad(const osm_depth_desc* d, const float* x0, const float* z, const float* m, const double* fit, float* g,
                   void* stream);

/* the three launches from one call */
int osm_depth_loss_grad(const osm_depth_desc* d, const float* x0, const float* z, const float* m, double* part, double* fit,
                        float* depth_loss, float* g, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_DEPTHPRIOR_H */
