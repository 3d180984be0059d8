/* osmosis_physgroup.h -- shared water / haze parameters across a burst: the grouped phi step of libosmosis_hip.so, the fifth
 * header of the library's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with
 * osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream; osm_phys_desc,
 * phi [B][9], red [B][16], part and opt_state [B][20] are the ones of the osm_phys_* family there) and osmosis_physlin.h (the data
 * term through a linear operator).  Strict C99.
 *
 * The B images of a call are partitioned into G contiguous groups, off[0] = 0 < off[1] < ... < off[G] = B; group j is the images
 * off[j] .. off[j + 1] - 1, photos of ONE water body.  All rows of a group carry the same phi and the same optimizer state (the
 * caller initialises them so; every step keeps them so).  Everything per image stays per image: red[b], loss_out[b], the loss
 * L_b (norm or mse), its gscale_b, the zero guard of the masked / composed paths, and with them the x0-gradient osm_phys_grad*
 * forms for the phi in hand -- they are osm_phys_finalize's (_m, _lin) bits.  The group's objective is the sum of its members'
 * total losses, so its gradient of a parameter is
 *
 *   omega * sum over the members b in ascending order of d_b ,  d_b = image b's gradient as osm_phys_finalize forms it in fp64
 *                                                                (the raw sums tot_b mapped onto the live parameters of `kind`,
 *                                                                times gscale_b; 0 for a zero-guarded member)
 *
 * summed in fp64 and cast to fp32 once; omega = 1 / n (reduce 1, mean: n the group's size, masked-out members included -- the step
 * sizes eta were chosen for one image's gradient) or 1 (reduce 0, sum).  ONE optimizer step per group (every optimizer code of
 * osm_phys_desc) moves phi and the state, and every member row receives the new values.  A group whose members are all
 * zero-guarded takes no step.  Fixed order, no atomics: results are bit-reproducible, a group's results do not depend on the other
 * groups of the call, and with every group of size 1 each entry point below IS its ungrouped counterpart, bit for bit, for both
 * `reduce` values. */
#ifndef OSMOSIS_PHYSGROUP_H
#define OSMOSIS_PHYSGROUP_H

#include "osmosis_hip.h"
#include "osmosis_physlin.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSM_MAX_GROUPS 64

typedef struct osm_group_desc {
  int G;            /* 1 .. OSM_MAX_GROUPS */
  const int* off;   /* HOST, [G + 1]: read when the entry point is called (the offsets travel in the kernel's arguments) */
  int reduce;       /* 0 sum, 1 mean */
} osm_group_desc;

/* osm_phys_finalize_m with one phi step per group (masked != 0: the zero guard) */
int osm_phys_finalize_g(const osm_phys_desc* d, const osm_group_desc* grp, const float* part, float* red, float* phi, int do_update,
                        float* loss_out, float* opt_state, int masked, void* stream);
/* osm_phys_finalize_lin with one phi step per group */
int osm_phys_finalize_lin_g(const osm_phys_desc* d, const osm_group_desc* grp, int hw, const float* part, const float* part_r, float* red,
                            float* phi, int do_update, float* loss_out, float* opt_state, int masked, void* stream);
/* osm_phys_optimize_m with one phi step per group and inner iteration: the launches of osm_phys_optimize_m, the grouped finalize
 * in the place of the plain one */
int osm_phys_optimize_g(const osm_phys_desc* d, const osm_group_desc* grp, const float* x0, const float* y, const float* mask /* NULL ok */,
                        float* phi, float* part, float* red, float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state,
                        void* stream);
/* osm_phys_optimize_lin likewise */
int osm_phys_optimize_lin_g(const osm_phys_desc* d, const osm_group_desc* grp, const osm_lin_desc* lin, const float* x0, const float* y,
                            const float* mask /* NULL ok */, float* phi, float* F, float* AF, float* u, float* v, float* part_r, float* part,
                            float* red, float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_PHYSGROUP_H */
