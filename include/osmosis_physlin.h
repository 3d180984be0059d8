/* osmosis_physlin.h -- the water / haze data term through a linear measurement operator (blur, super-resolution, a PSF) of
 * libosmosis_hip.so: the fourth header of the library's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a
 * negative osm_status on failure with osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t,
 * NULL = default stream; osm_phys_desc, phi [B][9], red [B][16], part and opt_state are the ones of the osm_phys_* family there),
 * osmosis_linop.h and osmosis_psf.h (the operators themselves).  Strict C99.
 *
 * The model: the photo in [0, 1] is A I, I_c = J_c exp(-phi_a d) + phi_inf (1 - exp(-phi_b d)) on the image grid [H,W], A applied
 * per plane with the measurement on A's own grid [h,w].  With w the depth weight of the descriptor (weight_type 1; a constant of
 * the step) and M the optional validity mask [B,3,hw]:
 *
 *   It = A I [B,3,hw] ;  wt = A w [B,1,hw] (weight_type 0: wt = 1, no weight plane is formed)
 *   r_c = (y_c - (2 It_c - 1)) wt M_c ;  S = sum r^2 per image
 *   norm: L = sqrt(S), gscale = 1 / L ;  mse: L = S / (3 h w), gscale = 2 / (3 h w)      (the measurement's size, not the image's)
 *   u_c = -2 wt M_c r_c [B,3,hw] ;  v = A^T u [B,3,HW]
 *   raw phi-gradient sums (red[1..9]): those of osm_phys_reduce with v_c in the place of its k2 = -2 w r_c
 *   dL/dI_c = gscale v_c ;  g = dL/dx0 follows as in osm_phys_grad, auxiliary losses (red[10..13], on the image grid) included
 *
 * Note 2 (A I) - 1, not A (2 I - 1): an operator whose gain is not 1 (an unnormalised PSF) means what it says.  With A the identity
 * this is the loss of osm_phys_optimize_m.  An image whose S is exactly 0 under the norm loss has no data-term gradient and takes
 * no phi step when `masked` is set (osm_phys_optimize_lin: mask != NULL), as osm_phys_finalize_m guards.
 * Every reduction runs in a fixed order through per-workgroup partial slots, no atomics: results are bit-reproducible and do not
 * depend on the batch an image travels in. */
#ifndef OSMOSIS_PHYSLIN_H
#define OSMOSIS_PHYSLIN_H

#include "osmosis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One operator A: [H,W] -> [h,w] per plane, tables / taps on the device. */
typedef struct osm_lin_desc {
  int family;                 /* 0 separable (osm_linop_apply), 1 psf (osm_psf_apply; h = H, w = W) */
  int H, W, h, w;
  /* family 0: the band tables of A (start_h [h], wt_h [h][Kh], start_w [w], wt_w [w][Kw]) and of its transpose
   * (tstart_h [H], twt_h [H][tKh], tstart_w [W], twt_w [W][tKw]) */
  const int* start_h;
  const float* wt_h;
  const int* start_w;
  const float* wt_w;
  int Kh, Kw;
  const int* tstart_h;
  const float* twt_h;
  const int* tstart_w;
  const float* twt_w;
  int tKh, tKw;
  /* family 1: the tap list dy [T], dx [T], tap_w [T] and its reach Ry, Rx */
  const int* dy;
  const int* dx;
  const float* tap_w;
  int T, Ry, Rx;
} osm_lin_desc;

/* Workspaces, P = 4 when d->weight_type == 1, else 3:
 *   F [B,P,HW]   planes 0..2 the image I_c (one fused multiply-add: fma(J, Ea, phi_inf (1 - Eb))), plane 3 the weight w
 *   AF [B,P,hw]  A F ;  u [B,3,hw] ;  v [B,3,HW] ;  part_r [B][osm_phys_nblk(hw)] ;  part [B][osm_phys_nblk(HW)][16]
 * d->kind must be 0, 1 or 2. */
int osm_phys_forward(const osm_phys_desc* d, const float* x0, const float* phi, float* F, void* stream);
/* u and the per-workgroup partial sums of r^2 from AF, y [B,3,hw] and mask [B,3,hw] (NULL: none) */
int osm_phys_resid(const osm_phys_desc* d, int hw, const float* AF, const float* y, const float* mask, float* u, float* part_r,
                   void* stream);
/* slots 1..13 of part from x0, phi and v (slot 0 is written as 0: osm_phys_finalize_lin takes it from part_r) */
int osm_phys_reduce_lin(const osm_phys_desc* d, const float* x0, const float* phi, const float* v, float* part, void* stream);
/* osm_phys_finalize_m with red[0] = sum part_r and n = 3 hw */
int osm_phys_finalize_lin(const osm_phys_desc* d, int hw, const float* part, const float* part_r, float* red, float* phi,
                          int do_update, float* loss_out, float* opt_state, int masked, void* stream);
/* g [B,4,HW] = d (total loss) / d x0 from v and the reductions in red */
int osm_phys_grad_lin(const osm_phys_desc* d, int hw, const float* x0, const float* phi, const float* v, const float* red, float* g,
                      int masked, void* stream);
/* The inner phi loop of one guided step in one call: n_inner x { forward; A (P planes); resid; A^T (3 planes); reduce_lin;
 * finalize_lin with the phi step }, the loss (loss_out [B]) and g taken at the phi of the last iteration (with that iteration's v),
 * which is stepped afterwards; freeze_phi != 0 (n_inner must be 1): loss and g only.  lin->H * lin->W must equal d->HW. */
int osm_phys_optimize_lin(const osm_phys_desc* d, const osm_lin_desc* lin, const float* x0, const float* y, const float* mask /* NULL ok */,
                          float* phi, float* F, float* AF, float* u, float* v, float* part_r, float* part, float* red, float* loss_out,
                          float* g, int n_inner, int freeze_phi, float* opt_state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_PHYSLIN_H */
