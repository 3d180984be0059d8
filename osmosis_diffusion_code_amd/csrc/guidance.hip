// Per-step sampler math outside the UNet (NCHW [B,4,H,W] like the reference's tensors):
//   posterior mean / x0 / log-variance            posterior_mean_variance.py:127-136, 246-258
//   physical image-formation model + guidance loss  measurements.py:138-151, 251-264, 363-376;
//                                                   condition_methods.py:109-144; losses.py:29-83
//   analytic gradient of that loss w.r.t. x0 and phi, on-device SGD on phi (measurements.py:266-303)
//   guidance update + ancestral noise               condition_methods.py:211-224; gaussian_diffusion.py:266-268
// All HBM/latency bound and tiny (a few MB per step); the point of doing them here is that the
// 20-iteration phi loop runs with no host synchronisation (the reference syncs 4+20 times a step).
// Batch semantics: every reduction is PER IMAGE (equal to B=1 reference runs image by image,
// SURVEY.md F1/F2).
// One kernel per job.  The step kernels (posterior, posterior_bwd, guide_update(_rng), ddim_update) take the state's C and the
// network output's Cout as launch arguments: the RGBD entry points pass (4, 8), the `_c` ones the RGB family's (3, 6) / (3, 3).
// The physics kernels are templates over what a route adds -- phys_reduce_kernel / phys_grad_kernel<MASKED, LIN> (a validity
// mask; a linear operator between the model and the residual), phys_finalize(_group)_kernel<LIN> over one shared device body --
// and ONE host function, phys_optimize_launch, enqueues the inner loop of the plain, masked, grouped and composed entry points.
#include "osm_common.h"
#include "depth_conv.h"
#include "../../include/osmosis_linop.h"
#include "../../include/osmosis_psf.h"
#include "../../include/osmosis_physlin.h"
#include "../../include/osmosis_physgroup.h"
#include "../../include/osmosis_solver.h"

namespace {

constexpr int PPB = 1024;  // pixels per reduce workgroup
constexpr int NRED = 16;

// MASKED: a per-pixel validity / confidence map M [B,3,HW] in [0, 1] (the layout of y) scales the residual: the effective weight of
// channel c is wm[c] = w M_c wherever the unmasked code uses w (the residual, k2 and dLdI).  The `false` instantiations carry no
// wm and are the unmasked code.
template <bool MASKED> struct PixMask { float wm[3]; };
template <> struct PixMask<false> {};

template <bool MASKED>
struct Pix : PixMask<MASKED> {
  float rgb[3], D, y[3];
  float d, dd, w;
  float Ea[3], Eb[3], J[3], r[3];
};

// FMA_I (the masked gradient kernel): J Ea + pinf (1 - Eb) with its one fused multiply-add spelled out -- the contraction the unmasked
// gradient kernel compiles to on every channel; left to the compiler, the masked kernel's extra multiplies changed what got packed
// and one channel lost the fusion, so M = 1 was one ulp off the unmasked gradient.
// MODEL_ONLY (the composed path, where a linear operator stands between the model and the residual): no measurement is read, y and
// mask may be null, and r[c] carries the image I_c itself.
template <bool MASKED, bool FMA_I = false, bool MODEL_ONLY = false>
__device__ __forceinline__ void eval_pixel(const osm_phys_desc& ds, const float* __restrict__ x0,
                                           const float* __restrict__ y, const float* __restrict__ mask,
                                           const float* __restrict__ phi, int b, int p, Pix<MASKED>& q) {
  const long long base = (long long)b * 4 * ds.HW + p;
  float m[3] = {1.f, 1.f, 1.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q.rgb[c] = x0[base + (long long)c * ds.HW];
    if constexpr (!MODEL_ONLY) q.y[c] = y[(long long)b * 3 * ds.HW + (long long)c * ds.HW + p];
    if constexpr (MASKED) m[c] = mask[(long long)b * 3 * ds.HW + (long long)c * ds.HW + p];
  }
  q.D = x0[base + 3LL * ds.HW];
  if (ds.kind == 3) {   // identity forward model of the rgb-guidance ('ps') path: I = x0[:, 0:3], unweighted (condition_methods.py:35-41)
    q.d = 0.f; q.dd = 0.f; q.w = 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      q.Ea[c] = q.Eb[c] = 1.f;
      q.J[c] = 0.5f * (q.rgb[c] + 1.0f);
      q.r[c] = q.y[c] - q.rgb[c];
      if constexpr (MASKED) { q.wm[c] = m[c]; q.r[c] *= m[c]; }
    }
    return;
  }
  q.d = conv_depth(q.D, ds.depth_type, ds.dval, q.dd);
  float wdd;
  q.w = ds.weight_type == 1 ? conv_depth(q.D, ds.wdepth_type, ds.wval, wdd) : 1.0f;
  const float* ph = phi + b * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float pa = ds.kind == 2 ? ph[0] : ph[c];
    const float pb = ds.kind == 0 ? ph[3 + c] : pa;
    const float pinf = ph[6 + c];
    q.Ea[c] = expf(-pa * q.d);
    q.Eb[c] = expf(-pb * q.d);
    q.J[c] = 0.5f * (q.rgb[c] + 1.0f);
    float I;
    if constexpr (FMA_I) {
      I = fmaf(q.J[c], q.Ea[c], pinf * (1.0f - q.Eb[c]));
    } else {
      I = q.J[c] * q.Ea[c] + pinf * (1.0f - q.Eb[c]);
    }
    if constexpr (MODEL_ONLY) {
      q.r[c] = I;
    } else if constexpr (MASKED) {
      q.wm[c] = q.w * m[c];
      q.r[c] = (q.y[c] - (2.0f * I - 1.0f)) * q.wm[c];
    } else {
      q.r[c] = (q.y[c] - (2.0f * I - 1.0f)) * q.w;
    }
  }
}

// LIN (the composed data term, a linear operator A between the model and the residual; include/osmosis_physlin.h): k2 is read from
// v = A^T u [B,3,HW] where the plain instantiations form -2 w r inline, no measurement is read (y and mask are null), and slot 0 of `part`
// is written as 0 (the finalize takes the squared residual from part_r, on the measurement's grid).
template <bool MASKED, bool LIN>
__global__ __launch_bounds__(256) void phys_reduce_kernel(osm_phys_desc ds, const float* __restrict__ x0,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ mask,
                                                           const float* __restrict__ phi, const float* __restrict__ v,
                                                           float* __restrict__ part, int nblk) {
  static_assert(!(MASKED && LIN), "the composed route's mask acts on the measurement's grid (phys_resid_kernel)");
  __shared__ float red[4][NRED];
  const int b = blockIdx.y, blk = blockIdx.x;
  float s[NRED];
#pragma unroll
  for (int k = 0; k < NRED; ++k) s[k] = 0.f;
  const int pend = min(ds.HW, (blk + 1) * PPB);
  const float* ph = phi + b * 9;
  for (int p = blk * PPB + threadIdx.x; p < pend; p += 256) {
    Pix<MASKED> q;
    eval_pixel<MASKED, false, LIN>(ds, x0, y, mask, phi, b, p, q);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float pinf = ph[6 + c];
      float k2;                                              // r_c * d r_c / d I_c
      if constexpr (LIN) {
        k2 = v[((long long)b * 3 + c) * ds.HW + p];
      } else {
        float wc = q.w;
        if constexpr (MASKED) wc = q.wm[c];
        k2 = -2.0f * wc * q.r[c];
        s[0] += q.r[c] * q.r[c];
      }
      s[1 + c] += k2 * (-q.d * q.J[c] * q.Ea[c]);            // d I / d phi_a
      s[4 + c] += k2 * (pinf * q.d * q.Eb[c]);               // d I / d phi_b
      s[7 + c] += k2 * (1.0f - q.Eb[c]);                     // d I / d phi_inf
      s[10 + c] += q.rgb[c];
      const float e = fmaxf(fabsf(q.rgb[c]) - 0.7f, 0.0f);
      s[13] += e * e;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NRED; ++k) {
    const float t = osm::wave_sum(s[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NRED) {
    const int k = threadIdx.x;
    part[((long long)b * nblk + blk) * NRED + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

__device__ __forceinline__ float sgn(float v) { return (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f); }

// The learning rate of every phi slot and the live mask of `kind` (bit i: phi[i] is a parameter of this operator).
__device__ __forceinline__ int phys_param_lr(const osm_phys_desc& ds, float* lr) {
  for (int i = 0; i < 9; ++i) lr[i] = 0.f;
  int live;
  if (ds.kind == 0) {
    for (int c = 0; c < 3; ++c) { lr[c] = ds.eta[0]; lr[3 + c] = ds.eta[1]; }
    live = 0x3f;
  } else if (ds.kind == 1) {
    for (int c = 0; c < 3; ++c) lr[c] = ds.eta[0];
    live = 0x7;
  } else {
    lr[0] = ds.eta[0];
    live = 0x1;
  }
  for (int c = 0; c < 3; ++c) lr[6 + c] = ds.eta[2];
  return live | 0x1c0;
}

// One image's gradient of every live parameter (as the reference's autograd leaves have it) from its reduced sums, in fp64: the
// plain finalize casts it to fp32 as it is, the grouped one sums it over the members of a group first.
__device__ __forceinline__ void phys_param_grad(const osm_phys_desc& ds, const double* tot, double gscale, double* dg) {
  for (int i = 0; i < 9; ++i) dg[i] = 0.0;
  if (ds.kind == 0) {
    for (int c = 0; c < 3; ++c) {
      dg[c] = tot[1 + c] * gscale;
      dg[3 + c] = tot[4 + c] * gscale;
    }
  } else if (ds.kind == 1) {
    for (int c = 0; c < 3; ++c) dg[c] = (tot[1 + c] + tot[4 + c]) * gscale;
  } else {
    double gs = 0.0;
    for (int c = 0; c < 3; ++c) gs += tot[1 + c] + tot[4 + c];
    dg[0] = gs * gscale;
  }
  for (int c = 0; c < 3; ++c) dg[6 + c] = tot[7 + c] * gscale;
}

// One optimizer step of one phi row ph [9] with its state row st [20] (NULL for sgd): shared by the per-image and the grouped
// finalize kernels.
__device__ __forceinline__ void phys_opt_step(const osm_phys_desc& ds, const float* g, const float* lr, int live, float* ph, float* st) {
  // torch.optim with its DEFAULT hyper-parameters (utils.py:494-524 passes none), single-tensor path, fp32 state, one parameter
  // group per phi with lr = eta (measurements.py:132-136, 244-249).  st: [B][20] floats, layout per optimizer below.  A parameter
  // with learn_flag False has no gradient: the optimizer skips it (its state stays untouched).
  if (ds.optimizer == 1 || ds.optimizer == 2) {          // Adam | AdamW (weight_decay 0.01, decoupled): exp_avg[9] | exp_avg_sq[9] | step
    const float step = st[18] + 1.f;
    st[18] = step;
    const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    const float bc2_sqrt = (float)sqrt(bc2);
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      if (ds.optimizer == 2) ph[i] *= (float)(1.0 - (double)lr[i] * 0.01);      // param.mul_(1 - lr * weight_decay)
      const float m = st[i] + (g[i] - st[i]) * (float)(1.0 - b1);             // exp_avg.lerp_(grad, 1 - beta1)
      const float v = st[9 + i] * (float)b2 + (float)(1.0 - b2) * g[i] * g[i];  // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
      st[i] = m; st[9 + i] = v;
      const float denom = sqrtf(v) / bc2_sqrt + (float)eps;
      ph[i] += (float)(-(double)lr[i] / bc1) * (m / denom);                   // param.addcdiv_(exp_avg, denom, value=-step_size)
    }
  } else if (ds.optimizer == 3) {   // Adamax (betas 0.9 / 0.999, eps 1e-8): exp_avg[9] | exp_inf[9] | step
    const float step = st[18] + 1.f;
    st[18] = step;
    const double bc = 1.0 - pow(0.9, (double)step);
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      const float m = st[i] + (g[i] - st[i]) * (float)(1.0 - 0.9);            // exp_avg.lerp_(grad, 1 - beta1)
      const float u = fmaxf(st[9 + i] * (float)0.999, fabsf(g[i]) + (float)1e-8);   // max(exp_inf * beta2, |grad| + eps)
      st[i] = m; st[9 + i] = u;
      ph[i] += (float)(-(double)lr[i] / bc) * (m / u);                         // param.addcdiv_(exp_avg, exp_inf, value=-clr)
    }
  } else if (ds.optimizer == 4) {   // RMSprop (alpha 0.99, eps 1e-8, no momentum, not centered): square_avg[9]
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      const float sq = st[i] * (float)0.99 + (float)(1.0 - 0.99) * g[i] * g[i];
      st[i] = sq;
      ph[i] += -lr[i] * (g[i] / (sqrtf(sq) + (float)1e-8));
    }
  } else if (ds.optimizer == 5) {   // Adagrad (lr_decay 0, initial accumulator 0, eps 1e-10): sum[9]
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      const float sm = st[i] + g[i] * g[i];
      st[i] = sm;
      ph[i] += -lr[i] * (g[i] / (sqrtf(sm) + (float)1e-10));
    }
  } else if (ds.optimizer == 6) {   // Adadelta (rho 0.9, eps 1e-6; lr = eta): square_avg[9] | acc_delta[9]
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      const float sq = st[i] * (float)0.9 + (float)(1.0 - 0.9) * g[i] * g[i];
      const float sd = sqrtf(sq + (float)1e-6);
      const float dl = sqrtf(st[9 + i] + (float)1e-6) / sd * g[i];
      st[i] = sq;
      st[9 + i] = st[9 + i] * (float)0.9 + (float)(1.0 - 0.9) * dl * dl;
      ph[i] += -lr[i] * dl;
    }
  } else if (ds.optimizer == 7) {   // ASGD (lambd 1e-4, alpha 0.75, t0 1e6): eta[9] | - | step (19); eta starts at lr (0 = not yet set)
    const float step = st[19] + 1.f;
    st[19] = step;
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      const float eta = step == 1.f ? lr[i] : st[i];
      ph[i] *= (float)(1.0 - 1e-4 * (double)eta);                             // param.mul_(1 - lambd * eta)
      ph[i] += -eta * g[i];                                                    // param.add_(grad, alpha=-eta)
      st[i] = (float)((double)lr[i] / pow(1.0 + 1e-4 * (double)lr[i] * (double)step, 0.75));
    }                                                                          // (the averaged iterate `ax` is not what the operator reads)
  } else if (ds.optimizer == 8) {   // Rprop (etas 0.5 / 1.2, step sizes 1e-6 .. 50): prev[9] | step_size[9] | step
    const float step = st[18] + 1.f;
    st[18] = step;
    for (int i = 0; i < 9; ++i) {
      if (!((live >> i) & 1) || lr[i] == 0.f) continue;
      float ss = step == 1.f ? lr[i] : st[9 + i];
      const float pr = g[i] * st[i];
      float gi = g[i];
      ss *= pr > 0.f ? 1.2f : (pr < 0.f ? 0.5f : 1.f);
      ss = fminf(fmaxf(ss, 1e-6f), 50.f);
      if (pr < 0.f) gi = 0.f;
      ph[i] += -(sgn(gi) * ss);
      st[i] = gi; st[9 + i] = ss;
    }
  } else {
    for (int i = 0; i < 9; ++i)
      if ((live >> i) & 1) ph[i] -= lr[i] * g[i];
  }
  if (ds.kind == 2) ph[1] = ph[2] = ph[0];
}

// The finalize of one reduce: per image the NRED sums (red) and the loss, then one optimizer step of phi.  Its three parts exist
// once, as device functions; two thin kernels call them (ONE kernel with the per-image launch as its identity grouping measured
// 6.2 us per launch against 4.4 - 4.7 us on the per-image path, which runs 21 times a step: it paid the group kernel's shared-memory
// round trip and two more barriers).
// LIN (the composed path): component 0, the sum of squared residuals, comes from lin.part_r [B][lin.nblk_r] -- the residual lives
// on the measurement's grid of lin.hw pixels -- and the losses normalise by that grid.  The `false` instantiation carries no such
// argument.
template <bool LIN> struct FinLin { const float* part_r; int nblk_r, hw; };
template <> struct FinLin<false> {};

// One wave walks image b's nblk partials into tot [NRED] (shared) and red[b]: component lane >> 2, four lanes share its partials
// (fixed order: deterministic), fp64, two shuffle folds (a single lane per component walked 64 dependent loads: 10.6 us per
// launch, 21 launches per step)
template <bool LIN>
__device__ __forceinline__ void fin_walk(const float* __restrict__ part, float* __restrict__ red, int nblk, const FinLin<LIN>& lin,
                                         int b, int lane, double* tot) {
  static_assert(NRED * 4 == 64, "one wave covers the components");
  const int comp = lane >> 2, sub = lane & 3;
  double a = 0.0;
#pragma unroll 4
  for (int k = sub; k < nblk; k += 4) a += (double)part[((long long)b * nblk + k) * NRED + comp];
  if constexpr (LIN) {
    if (comp == 0) {
      a = 0.0;
      for (int k = sub; k < lin.nblk_r; k += 4) a += (double)lin.part_r[(long long)b * lin.nblk_r + k];
    }
  }
  a += __shfl_xor(a, 1, 64);
  a += __shfl_xor(a, 2, 64);
  if (sub == 0) {
    tot[comp] = a;
    red[b * NRED + comp] = (float)a;
  }
}

// One lane, after the walk's barrier: image b's loss and, for a step, its fp64 parameter gradient dg [9].  Returns whether the
// image steps: not on the masked path (zero_guard) with every pixel masked out -- the data term has no gradient there
// (torch.linalg.norm's backward at 0; dg is 0) and does not step phi (no optimizer state moves either).
template <bool LIN>
__device__ __forceinline__ bool fin_member(const osm_phys_desc& ds, const double* tot, const FinLin<LIN>& lin, int zero_guard, int b,
                                           float* __restrict__ loss_out, int do_update, double* dg) {
  double n = 3.0 * (double)ds.HW;
  if constexpr (LIN) n = 3.0 * (double)lin.hw;
  double L, gscale;
  bool live = true;
  if (ds.loss_type == 0) {
    L = sqrt(tot[0]);
    gscale = 1.0 / L;
    if (zero_guard && tot[0] == 0.0) { gscale = 0.0; live = false; }
  } else {
    L = tot[0] / n;
    gscale = 2.0 / n;
  }
  if (loss_out) loss_out[b] = (float)L;
  if (do_update) phys_param_grad(ds, tot, gscale, dg);
  return live;
}

// One lane: the optimizer step of the row ph (state row st, NULL for sgd) with the fp64 gradient omega dg
__device__ __forceinline__ void fin_step(const osm_phys_desc& ds, const double* dg, double omega, float* ph, float* st) {
  float g[9], lr[9];
  const int live = phys_param_lr(ds, lr);
  for (int i = 0; i < 9; ++i) g[i] = (float)(dg[i] * omega);
  phys_opt_step(ds, g, lr, live, ph, st);
}

// Per image: one wave per image, grid B
template <bool LIN>
__global__ void phys_finalize_kernel(osm_phys_desc ds, const float* __restrict__ part, float* __restrict__ red,
                                     float* __restrict__ phi, int do_update, float* __restrict__ loss_out,
                                     float* __restrict__ opt_state, int nblk, int zero_guard, const FinLin<LIN> lin) {
  __shared__ double tot[NRED];
  const int b = blockIdx.x;
  fin_walk(part, red, nblk, lin, b, threadIdx.x, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    double dg[9];
    if (fin_member(ds, tot, lin, zero_guard, b, loss_out, do_update, dg) && do_update)
      fin_step(ds, dg, 1.0, phi + b * 9, opt_state ? opt_state + b * 20 : nullptr);
  }
}

// Per group (include/osmosis_physgroup.h): the images off[g] .. off[g + 1] - 1 share ONE phi row and ONE optimizer state row.  One
// workgroup per group, its members dealt to the GWAVES waves round by round; a wave does for its member what the per-image
// kernel's single wave does (red[b] and loss_out[b] are its bits), lane 0 leaves the member's gradient in shared memory, and thread
// 0 adds the members up in ascending order, starting FROM the first member's -- fixed order, no atomics; the addends come out of
// shared memory, so no multiply is contracted into the sum and a + a is exact.  Then one optimizer step on the group's first row
// with omega * sum (omega = 1 / n for `mean`, 1 for `sum`), and every other member row receives the new phi and state.  A member
// that is zero-guarded adds zeros; a group whose members are all guarded takes no step.  With n = 1 the sum is the member's own
// gradient and omega = 1: phys_finalize_kernel bit for bit, signed zeros included.
struct GroupOff { int G, reduce_mean, off[OSM_MAX_GROUPS + 1]; };
constexpr int GWAVES = 4;

template <bool LIN>
__global__ __launch_bounds__(64 * GWAVES) void phys_finalize_group_kernel(osm_phys_desc ds, const float* __restrict__ part,
                                                                          float* __restrict__ red, float* phi, int do_update,
                                                                          float* __restrict__ loss_out, float* opt_state, int nblk,
                                                                          int zero_guard, const GroupOff go, const FinLin<LIN> lin) {
  __shared__ double tot[GWAVES][NRED];
  __shared__ double dsh[GWAVES][9];
  __shared__ int live_sh[GWAVES];
  __shared__ float row[9 + 20];
  __shared__ int stepped;
  const int b0 = go.off[blockIdx.x], n = go.off[blockIdx.x + 1] - b0;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc[9];                                                     // thread 0: the group's sum
  int any = 0;                                                       // thread 0: a member that is not zero-guarded
  for (int r0 = 0; r0 < n; r0 += GWAVES) {
    const int m = r0 + wv;                // this wave's member of the round (wave-uniform)
    if (m < n) fin_walk(part, red, nblk, lin, b0 + m, lane, tot[wv]);
    __syncthreads();
    if (m < n && lane == 0) live_sh[wv] = fin_member(ds, tot[wv], lin, zero_guard, b0 + m, loss_out, do_update, dsh[wv]);
    __syncthreads();
    if (threadIdx.x == 0 && do_update) {
      const int cnt = min(GWAVES, n - r0);
      for (int w = 0; w < cnt; ++w) {
        for (int i = 0; i < 9; ++i) acc[i] = r0 + w == 0 ? dsh[w][i] : acc[i] + dsh[w][i];
        any |= live_sh[w];
      }
    }
    // (the next round writes tot / dsh only after its own barriers, which thread 0 reaches after this sum)
  }
  if (threadIdx.x == 0) {
    stepped = 0;
    if (do_update && any) {
      float* ph = phi + b0 * 9;
      float* st = opt_state ? opt_state + b0 * 20 : nullptr;
      fin_step(ds, acc, go.reduce_mean ? 1.0 / (double)n : 1.0, ph, st);
      for (int i = 0; i < 9; ++i) row[i] = ph[i];
      for (int i = 0; i < 20; ++i) row[9 + i] = st ? st[i] : 0.f;
      stepped = 1;
    }
  }
  __syncthreads();
  if (stepped) {      // every other member row receives the group's new phi and state
    for (int idx = threadIdx.x; idx < (n - 1) * 29; idx += 64 * GWAVES) {
      const int b = b0 + 1 + idx / 29, k = idx % 29;
      if (k < 9) phi[b * 9 + k] = row[k];
      else if (opt_state) opt_state[b * 20 + (k - 9)] = row[k];
    }
  }
}

// ---------------------------------------------------------------- the Levenberg-Marquardt phi solver (osm_phys_desc.optimizer = 9)
// The residual r_c = (y_c - (2 I_c - 1)) wm_c is linear in the image, and the image has three parameters per channel, with the
// model columns col_a = -d J_c Ea_c, col_b = phi_inf_c d Eb_c, col_i = 1 - Eb_c (d I_c / d phi).  The Jacobian of r is -2 wm col, so
// sums 1..9 of the plain reduce (sum k2 col, k2 = -2 wm r) are J^T r already, and J^T J is per channel the six entries
// aa, ab, ai, bb, bi, ii of sum 4 wm^2 col_p col_q: 18 more sums over the same pixel pass.
constexpr int NLM = 32;               // floats per reduce workgroup: the NRED slots of phys_reduce_kernel (0..13 used), then 18 Gram sums
constexpr int LM_GRAM = 14;           // slot of channel c's entry e (aa, ab, ai, bb, bi, ii): LM_GRAM + 6 c + e
constexpr int LM_STATE_S = 9, LM_STATE_LAMBDA = 10, LM_STATE_RETRY = 11;   // opt_state row: phi_base [9] | S_base | lambda | retry | reserved
constexpr double LM_LAMBDA0 = 1.0;                  // the lambda of a zero-initialised state row
constexpr double LM_LAMBDA_MIN = 1e-6, LM_LAMBDA_MAX = 1e6, LM_LAMBDA_FACTOR = 10.0;
constexpr double LM_ACCEPT_SLACK = 1e-5;            // accept iff S <= (1 + slack) S_base: converged ties do not flip on rounding
constexpr double LM_DIAG_EPS = 1e-12;               // the damping is lambda (diag A + eps max diag A): a dead column keeps a pivot

// Slots 0..13: phys_reduce_kernel's expressions in its order; the same tiling, wave sums and pairwise fold of the four waves.
template <bool MASKED>
__global__ __launch_bounds__(256) void phys_lm_reduce_kernel(osm_phys_desc ds, const float* __restrict__ x0,
                                                              const float* __restrict__ y, const float* __restrict__ mask,
                                                              const float* __restrict__ phi, float* __restrict__ part, int nblk) {
  __shared__ float red[4][NLM];
  const int b = blockIdx.y, blk = blockIdx.x;
  float s[NLM];
#pragma unroll
  for (int k = 0; k < NLM; ++k) s[k] = 0.f;
  const int pend = min(ds.HW, (blk + 1) * PPB);
  const float* ph = phi + b * 9;
  for (int p = blk * PPB + threadIdx.x; p < pend; p += 256) {
    Pix<MASKED> q;
    eval_pixel<MASKED, false, false>(ds, x0, y, mask, phi, b, p, q);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float pinf = ph[6 + c];
      float wc = q.w;
      if constexpr (MASKED) wc = q.wm[c];
      const float k2 = -2.0f * wc * q.r[c];
      const float ca = -q.d * q.J[c] * q.Ea[c], cb = pinf * q.d * q.Eb[c], ci = 1.0f - q.Eb[c];
      s[0] += q.r[c] * q.r[c];
      s[1 + c] += k2 * ca;
      s[4 + c] += k2 * cb;
      s[7 + c] += k2 * ci;
      s[10 + c] += q.rgb[c];
      const float e = fmaxf(fabsf(q.rgb[c]) - 0.7f, 0.0f);
      s[13] += e * e;
      const float w4 = 4.0f * wc * wc;
      const float wa = w4 * ca, wb = w4 * cb;
      s[LM_GRAM + 6 * c + 0] += wa * ca;
      s[LM_GRAM + 6 * c + 1] += wa * cb;
      s[LM_GRAM + 6 * c + 2] += wa * ci;
      s[LM_GRAM + 6 * c + 3] += wb * cb;
      s[LM_GRAM + 6 * c + 4] += wb * ci;
      s[LM_GRAM + 6 * c + 5] += w4 * ci * ci;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NLM; ++k) {
    const float t = osm::wave_sum(s[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NLM) {
    const int k = threadIdx.x;
    part[((long long)b * nblk + blk) * NLM + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

// The normal equations of image b over the live slots of phys_param_lr (a zero eta removes a slot; its value is otherwise ignored),
// assembled in fp64 from the totals: A [9][9] over the phi slots (kind 0: a block (a_c, b_c, i_c) per channel; kind 1: the column
// col_a + col_b in slot c; kind 2: slot 0 carries col_a + col_b of all three channels, an arrow with the three phi_inf), g = J^T r.
// Then (A + lambda (diag A + eps max diag A)) delta = -g by Cholesky on the live slots.  False: a non-positive pivot or a
// non-finite delta.
__device__ __forceinline__ bool lm_solve(const osm_phys_desc& ds, const double* tot, double lambda, double (*A)[9], double* delta) {
  float lr[9];
  const int mask = phys_param_lr(ds, lr);
  int idx[9], n = 0;
  for (int i = 0; i < 9; ++i)
    if (((mask >> i) & 1) && lr[i] != 0.f) idx[n++] = i;
  double g[9];
  for (int i = 0; i < 9; ++i) {
    g[i] = 0.0;
    delta[i] = 0.0;
    for (int j = 0; j < 9; ++j) A[i][j] = 0.0;
  }
  for (int c = 0; c < 3; ++c) {
    const double* G = tot + LM_GRAM + 6 * c;
    const double aa = G[0], ab = G[1], ai = G[2], bb = G[3], bi = G[4], ii = G[5];
    const int pi = 6 + c;
    if (ds.kind == 0) {
      const int pa = c, pb = 3 + c;
      A[pa][pa] = aa; A[pa][pb] = A[pb][pa] = ab; A[pa][pi] = A[pi][pa] = ai;
      A[pb][pb] = bb; A[pb][pi] = A[pi][pb] = bi;
      g[pa] = tot[1 + c]; g[pb] = tot[4 + c];
    } else {
      const int pa = ds.kind == 1 ? c : 0;
      A[pa][pa] += aa + 2.0 * ab + bb;
      A[pa][pi] += ai + bi;
      A[pi][pa] = A[pa][pi];
      g[pa] += tot[1 + c] + tot[4 + c];
    }
    A[pi][pi] = ii;
    g[pi] = tot[7 + c];
  }
  double dmax = 0.0;
  for (int k = 0; k < n; ++k) dmax = fmax(dmax, A[idx[k]][idx[k]]);
  for (int k = 0; k < n; ++k) A[idx[k]][idx[k]] += lambda * (A[idx[k]][idx[k]] + LM_DIAG_EPS * dmax);
  // Cholesky A = L L^T in place (lower triangle), on the live slots
  for (int k = 0; k < n; ++k) {
    const int p = idx[k];
    double dk = A[p][p];
    for (int m = 0; m < k; ++m) dk -= A[p][idx[m]] * A[p][idx[m]];
    if (!(dk > 0.0) || !isfinite(dk)) return false;
    dk = sqrt(dk);
    A[p][p] = dk;
    for (int r = k + 1; r < n; ++r) {
      const int q = idx[r];
      double v = A[q][p];
      for (int m = 0; m < k; ++m) v -= A[q][idx[m]] * A[p][idx[m]];
      A[q][p] = v / dk;
    }
  }
  double z[9];
  for (int k = 0; k < n; ++k) {          // L z = -g
    const int p = idx[k];
    double v = -g[p];
    for (int m = 0; m < k; ++m) v -= A[p][idx[m]] * z[m];
    z[k] = v / A[p][p];
  }
  for (int k = n - 1; k >= 0; --k) {     // L^T delta = z
    const int p = idx[k];
    double v = z[k];
    for (int m = k + 1; m < n; ++m) v -= A[idx[m]][p] * delta[idx[m]];
    delta[p] = v / A[p][p];
    if (!isfinite(delta[p])) return false;
  }
  return true;
}

// The LM finalize, one wave per image (lane 0 decides and solves), grid B.  mode (the entry points' do_update): 1 decide + step, 2 the same as the first
// iteration of a call (S_base is forgotten: x0 has changed), 3 close -- decide only, on the NRED sums of a plain reduce at the trial phi.
//   accept (no base yet, or S <= (1 + slack) S_base): base <- (phi, S); lambda <- lambda / 10 unless this was the re-evaluation after
//     a reject; then (modes 1, 2) phi <- phi_base + delta.  A failed solve counts as a reject at the new base.
//   reject (also a non-finite S or sum): lambda <- 10 lambda, phi <- phi_base, retry set, no step; the next iteration re-evaluates at
//     the base and steps with the larger lambda.  Close: red[0] and the loss become those of S_base.  With no base yet: no step,
//     the base stays unset (S_base = -1) and phi stays.
//   S == 0 (a fully masked image): phi and the state stay as they are.  J^T r == 0: no step.
// mode 1, 2 read NLM floats per workgroup of `part`, mode 3 reads NRED.
__global__ void phys_lm_finalize_kernel(osm_phys_desc ds, const float* __restrict__ part, float* __restrict__ red,
                                        float* __restrict__ phi, int mode, float* __restrict__ loss_out,
                                        float* __restrict__ opt_state, int nblk) {
  __shared__ double tot[NLM];
  __shared__ double A[9][9];
  const int b = blockIdx.x, lane = threadIdx.x;
  const bool close = mode == 3;
  if (close) {
    fin_walk(part, red, nblk, FinLin<false>{}, b, lane, tot);
  } else {              // component lane >> 1, two lanes share its partials (fixed order), fp64, one shuffle fold
    const int comp = lane >> 1, sub = lane & 1;
    double a = 0.0;
#pragma unroll 4
    for (int k = sub; k < nblk; k += 2) a += (double)part[((long long)b * nblk + k) * NLM + comp];
    a += __shfl_xor(a, 1, 64);
    if (sub == 0) {
      tot[comp] = a;
      if (comp < NRED) red[b * NRED + comp] = (float)a;
    }
  }
  __syncthreads();
  if (lane != 0) return;
  const double n3 = 3.0 * (double)ds.HW;
  double S = tot[0];
  float* ph = phi + b * 9;
  float* st = opt_state + b * 20;
  bool finite = isfinite(S);
  for (int k = 1; k < 10; ++k) finite = finite && isfinite(tot[k]);
  if (!close)
    for (int k = LM_GRAM; k < NLM; ++k) finite = finite && isfinite(tot[k]);
  bool restored = false;
  if (!(finite && S == 0.0)) {
    double lambda = (double)st[LM_STATE_LAMBDA];
    if (!(lambda > 0.0) || !isfinite(lambda)) lambda = LM_LAMBDA0;
    lambda = fmin(fmax(lambda, LM_LAMBDA_MIN), LM_LAMBDA_MAX);
    const bool nobase = mode == 2 || !(st[LM_STATE_S] > 0.f);     // (S == 0 never becomes a base: a zero row has none)
    const bool retry = st[LM_STATE_RETRY] != 0.f;
    bool reject;
    if (!finite) {
      reject = true;
    } else {
      reject = !(nobase || S <= (1.0 + LM_ACCEPT_SLACK) * (double)st[LM_STATE_S]);
    }
    if (!reject) {
      for (int i = 0; i < 9; ++i) st[i] = ph[i];
      st[LM_STATE_S] = (float)S;
      if (!retry) lambda = fmax(lambda / LM_LAMBDA_FACTOR, LM_LAMBDA_MIN);
      st[LM_STATE_RETRY] = 0.f;
      bool zero_g = true;
      for (int k = 1; k < 10; ++k) zero_g = zero_g && tot[k] == 0.0;
      if (!close && !zero_g) {
        double delta[9];
        bool ok = lm_solve(ds, tot, lambda, A, delta);
        float np[9];
        for (int i = 0; ok && i < 9; ++i) {
          np[i] = (float)((double)ph[i] + delta[i]);
          ok = isfinite(np[i]);
        }
        if (ok) {
          for (int i = 0; i < 9; ++i) ph[i] = np[i];
          if (ds.kind == 2) ph[1] = ph[2] = ph[0];
        } else {          // phi stays the base just taken
          lambda = fmin(lambda * LM_LAMBDA_FACTOR, LM_LAMBDA_MAX);
          st[LM_STATE_RETRY] = 1.f;
        }
      }
    } else if (nobase) {  // nothing to fall back to: phi stays, and the next iteration still has no base
      for (int i = 0; i < 9; ++i) st[i] = ph[i];
      st[LM_STATE_S] = -1.f;
      st[LM_STATE_RETRY] = 0.f;
    } else {
      lambda = fmin(lambda * LM_LAMBDA_FACTOR, LM_LAMBDA_MAX);
      for (int i = 0; i < 9; ++i) ph[i] = st[i];
      st[LM_STATE_RETRY] = 1.f;
      restored = true;
    }
    st[LM_STATE_LAMBDA] = (float)lambda;
  }
  if (close && restored) {
    S = (double)st[LM_STATE_S];
    red[b * NRED] = st[LM_STATE_S];
  }
  if (loss_out) loss_out[b] = (float)(ds.loss_type == 0 ? sqrt(S) : S / n3);
}

// LIN: dL/dI_c = v_c gscale with v = A^T u where the plain instantiations form -2 w r gscale inline; mse normalises by the measurement's
// 3 hw (the auxiliary losses by the image's 3 HW), and the zero guard of a fully masked image is the launch's flag (the mask lives
// on the measurement's grid, in phys_resid_kernel).
template <bool MASKED, bool LIN>
__global__ __launch_bounds__(256) void phys_grad_kernel(osm_phys_desc ds, const float* __restrict__ x0,
                                                         const float* __restrict__ y,
                                                         const float* __restrict__ mask,
                                                         const float* __restrict__ phi, const float* __restrict__ v,
                                                         const float* __restrict__ red, float* __restrict__ g, int hw,
                                                         int zero_guard) {
  static_assert(!(MASKED && LIN), "the composed route's mask acts on the measurement's grid (phys_resid_kernel)");
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ds.HW) return;
  Pix<MASKED> q;
  eval_pixel<MASKED, MASKED, LIN>(ds, x0, y, mask, phi, b, p, q);
  const float* rd = red + b * NRED;
  const float n = 3.0f * (float)ds.HW;
  float gscale = ds.loss_type == 0 ? 1.0f / sqrtf(rd[0]) : 2.0f / (LIN ? 3.0f * (float)hw : n);
  // a fully masked image: no data-term gradient (the auxiliary losses, which act on the prediction, remain)
  if ((MASKED || (LIN && zero_guard)) && ds.loss_type == 0 && rd[0] == 0.f) gscale = 0.f;
  const float* ph = phi + b * 9;
  float gD = 0.f;
  const long long base = (long long)b * 4 * ds.HW + p;
  if constexpr (!LIN) {   // (kind 3 has no model to compose with: the host refuses it on the composed route)
    if (ds.kind == 3) {   // d ||y - x0[:, 0:3]|| / d x0 = -(y - x0) / ||.|| on the colour channels, nothing on depth
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (MASKED) g[base + (long long)c * ds.HW] = -(q.wm[c] * (q.r[c] * gscale));
        else g[base + (long long)c * ds.HW] = -(q.r[c] * gscale);
      }
      g[base + 3LL * ds.HW] = 0.f;
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float pa = ds.kind == 2 ? ph[0] : ph[c];
    const float pb = ds.kind == 0 ? ph[3 + c] : pa;
    const float pinf = ph[6 + c];
    float dLdI;
    if constexpr (LIN) {
      dLdI = v[((long long)b * 3 + c) * ds.HW + p] * gscale;
    } else {
      float wc = q.w;
      if constexpr (MASKED) wc = q.wm[c];
      dLdI = -2.0f * wc * (q.r[c] * gscale);
    }
    float grgb = dLdI * 0.5f * q.Ea[c];
    if (ds.gamma_avrg != 0.f) grgb += ds.gamma_avrg * sgn(rd[10 + c]) / (float)ds.HW;
    if (ds.gamma_val != 0.f) {
      const float e = fmaxf(fabsf(q.rgb[c]) - 0.7f, 0.0f);
      grgb += ds.gamma_val * 2.0f * e * sgn(q.rgb[c]) / n;
    }
    g[base + (long long)c * ds.HW] = grgb;
    gD += dLdI * (-pa * q.J[c] * q.Ea[c] + pinf * pb * q.Eb[c]) * q.dd;
  }
  g[base + 3LL * ds.HW] = gD;
}

// ---------------------------------------------------------------- the data term through a linear operator A (blur, super-resolution)
// y = A I on A's own grid [h,w]: the image is materialised (forward), A applied (osm_linop_apply / osm_psf_apply), the residual taken on
// the measurement's grid (resid), A^T brings u = d S / d (A I) back (v), and the phi / x0 gradients read v where the kernels above form
// k2 = -2 w r inline (their LIN instantiations).  Reductions: fixed order through per-workgroup partial slots, no atomics.

// F [B,P,HW]: planes 0..2 the image I_c, plane 3 (P = 4, weight_type 1) the depth weight w
__global__ __launch_bounds__(256) void phys_forward_kernel(osm_phys_desc ds, const float* __restrict__ x0,
                                                            const float* __restrict__ phi, float* __restrict__ F, int P) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ds.HW) return;
  Pix<false> q;
  eval_pixel<false, true, true>(ds, x0, nullptr, nullptr, phi, b, p, q);
  const long long base = (long long)b * P * ds.HW + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) F[base + (long long)c * ds.HW] = q.r[c];
  if (P == 4) F[base + 3LL * ds.HW] = q.w;
}

// On the measurement's grid: r_c = (y_c - (2 (A I)_c - 1)) (A w) M_c, u_c = -2 (A w) M_c r_c, part_r[b][blk] = this workgroup's sum r^2
__global__ __launch_bounds__(256) void phys_resid_kernel(const float* __restrict__ AF, const float* __restrict__ y,
                                                          const float* __restrict__ mask, float* __restrict__ u,
                                                          float* __restrict__ part_r, int P, int hw, int nblk) {
  __shared__ float red[4];
  const int b = blockIdx.y, blk = blockIdx.x;
  float s = 0.f;
  const int pend = min(hw, (blk + 1) * PPB);
  for (int p = blk * PPB + threadIdx.x; p < pend; p += 256) {
    const float wt = P == 4 ? AF[((long long)b * P + 3) * hw + p] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long e = ((long long)b * 3 + c) * hw + p;
      const float wm = mask ? wt * mask[e] : wt;
      const float r = (y[e] - (2.0f * AF[((long long)b * P + c) * hw + p] - 1.0f)) * wm;
      u[e] = -2.0f * wm * r;
      s += r * r;
    }
  }
  const float t = osm::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part_r[(long long)b * nblk + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- posterior
// [B,C,HW] state, [B,Cout,HW] network output: the RGBD model (4, 8), the RGB model family (create_model with pretrain_model !=
// "osmosis": 3 -> 6, or 3 -> 3 without learn_sigma) and any C -> C model with a fixed variance.  Cout == C: the network has no
// variance half and the variance processor reads model_out itself (reference gaussian_diffusion.py:349-355, model_var_values =
// model_output).
// MK: mean processor (0 epsilon / start_x / previous_x through ONE form, x0 = c0 x - c1 out: the row holds
//     c0 = d x0 / d x and c1 = -d x0 / d out, which is also what posterior_bwd_kernel and the update kernels read;
//     1 start_x, x0 = out exactly; 2 previous_x, mean = out exactly).  VK: variance processor (0 learned_range,
//     1 fixed_small / fixed_large: the row's value, 2 learned: the network's second half).
// x0_raw != nullptr: clip_denoised (process_xstart, posterior_mean_variance.py:43-50): the unclamped prediction goes to x0_raw
// (clamp_bwd_kernel masks the guidance gradient with it), x0 = clamp(x0_raw, -1, 1) and the mean is formed from the clamped x0.
// RAW: the first pass of dynamic_threshold: the prediction to x0_raw, logvar, and the previous_x mean (= out); x0 and the other
// means wait for the batch-wide quantile (dynthr_apply_kernel).
template <int MK, int VK, bool RAW>
__global__ __launch_bounds__(256) void posterior_kernel(const float* __restrict__ mo, const float* __restrict__ x,
                                                           const float* __restrict__ coef, float* __restrict__ x0_raw,
                                                           float* __restrict__ x0, float* __restrict__ mean,
                                                           float* __restrict__ logvar, int B, int C, int Cout, int HW) {
  const long long n = (long long)C * HW, no = (long long)Cout * HW;
  const long long total = (long long)B * n;
  const long long voff = Cout == C ? 0 : n;
  const float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], mn = coef[4], mxl = coef[5];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / n;
    const long long rem = i - b * n;
    const float eps = mo[b * no + rem];
    const float xv = x[i];
    float xs = MK == 1 ? eps : c0 * xv - c1 * eps;
    if (RAW) {
      x0_raw[i] = xs;
      if (MK == 2) mean[i] = eps;
    } else {
      if (x0_raw) {
        x0_raw[i] = xs;
        xs = (xs != xs) ? xs : fminf(fmaxf(xs, -1.0f), 1.0f);          // torch.clamp keeps NaN
      }
      x0[i] = xs;
      mean[i] = MK == 2 ? eps : c2 * xs + c3 * xv;
    }
    if (VK == 1) {
      logvar[i] = mn;
    } else {
      const float v = mo[b * no + voff + rem];
      if (VK == 2) {
        logvar[i] = v;
      } else {
        const float frac = (v + 1.0f) / 2.0f;
        logvar[i] = frac * mxl + (1.0f - frac) * mn;
      }
    }
  }
}

// dynamic_threshold (util/img_utils.py:8-15): x0 = clip(q x0_raw, -1, 1) with q = quantile(|x0_raw|, s) over the whole batch (NaN
// kept, as torch.clip), then the mean from that x0 as posterior_kernel forms it (previous_x: the raw pass already wrote mean = out).
// A following clip_denoised clamp changes nothing.
template <int MK>
__global__ __launch_bounds__(256) void dynthr_apply_kernel(const float* __restrict__ x0_raw, const float* __restrict__ x,
                                                            const float* __restrict__ coef, const float* __restrict__ q,
                                                            float* __restrict__ x0, float* __restrict__ mean, long long total) {
  const float c2 = coef[2], c3 = coef[3], qv = q[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const float u = x0_raw[i] * qv;
    const float xs = (u != u) ? u : fminf(fmaxf(u, -1.0f), 1.0f);
    x0[i] = xs;
    if (MK != 2) {
      const float xv = x[i];
      mean[i] = c2 * xs + c3 * xv;
    }
  }
}

// backward of x.clamp(lo, hi) (ATen clamp_backward: the gradient passes where lo <= x <= hi, bounds included; NaN -> 0)
__global__ __launch_bounds__(256) void clamp_bwd_kernel(float* __restrict__ g, const float* __restrict__ x_raw, float lo, float hi,
                                                         long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v = x_raw[i];
    if (!(v >= lo && v <= hi)) g[i] = 0.f;
  }
}

// d_out[:, :C] = -c1 g, d_out[:, C:] = 0: exactly B * Cout * HW floats
__global__ __launch_bounds__(256) void posterior_bwd_kernel(const float* __restrict__ g, const float* __restrict__ coef,
                                                               float* __restrict__ d_out, int B, int C, int Cout, int HW) {
  const long long n = (long long)C * HW, no = (long long)Cout * HW;
  const long long total = (long long)B * no;
  const float c1 = coef[1];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / no;
    const long long rem = i - b * no;
    d_out[i] = rem < n ? -c1 * g[b * n + rem] : 0.f;
  }
}

__global__ __launch_bounds__(256) void guide_update_kernel(const float* __restrict__ mean, const float* __restrict__ logvar,
                                                              const float* __restrict__ g, const float* __restrict__ dxu,
                                                              const float* __restrict__ noise, const float* __restrict__ coef,
                                                              const float* __restrict__ scale, float clip,
                                                              float* __restrict__ x_next, float* __restrict__ grad_out, int B, int C,
                                                              int HW) {
  const long long total = (long long)B * C * HW;
  const float c0 = coef[0], noise_on = coef[6];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i / HW) % C);
    float grad = 0.f;
    if (g) grad = c0 * g[i] + (dxu ? dxu[i] : 0.f);
    if (grad_out) grad_out[i] = grad;
    float gc = grad;
    if (clip >= 0.f) gc = (grad != grad) ? grad : fminf(fmaxf(grad, -clip), clip);   // torch.clamp keeps NaN
    float xt = mean[i] - (g ? scale[c] * gc : 0.f);
    if (noise_on != 0.f && noise) xt += expf(0.5f * logvar[i]) * noise[i];
    x_next[i] = xt;
  }
}

// unconditional ancestral step of the RGBD prior sampler (reference osmosis_utils/diffusion.py:94-122):
//   eps = model_out[:, :C] ; x_next = c_a (x - c_b eps) + c_s z ; x0 = c_r x - c_m eps
// coef = {c_a, c_b, c_s, c_r, c_m, -, -, t}
__global__ __launch_bounds__(256) void ancestral_step_kernel(const float* __restrict__ mo,
                                                              const float* x,   // may alias x_next (in place)
                                                              const float* __restrict__ z,
                                                              const float* __restrict__ coef,
                                                              float* x_next, float* __restrict__ x0,
                                                              int B, int C, int Cout, int HW) {
  const long long total = (long long)B * C * HW;
  const float ca = coef[0], cb = coef[1], cs = coef[2], cr = coef[3], cm = coef[4];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / ((long long)C * HW);
    const long long rem = i - b * (long long)C * HW;
    const float eps = mo[b * (long long)Cout * HW + rem];
    const float xv = x[i];
    if (x0) x0[i] = cr * xv - cm * eps;
    float v = ca * (xv - cb * eps);
    if (z) v += cs * z[i];
    x_next[i] = v;
  }
}


// ---------------------------------------------------------------- step noise inside the library (gaussian_diffusion.py:266-268)
// Philox-4x32-10 (Salmon et al., SC'11; the Random123 constants), counter = (element quad, image, step | sub << 16, stream id),
// key = the 64-bit seed: one counter gives the four normals of four consecutive elements of one image (two Box-Muller pairs), so
// the noise of an image depends on (seed, image index, step, sub-step) only -- not on the batch it is processed in, its chunking
// or the grid.  sub: the repeat of a step at the same t (PCGS local_M, gaussian_diffusion.py:225-309); sub = 0 leaves word 2 = step.
struct Philox4 { unsigned v[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// (0, 1): 24 random bits, centred in their 2^-24 cell
__device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * 5.9604644775390625e-8f + 2.98023223876953125e-8f; }
__device__ __forceinline__ void normal4(const Philox4& r, float z[4]) {
  const float r0 = sqrtf(-2.0f * logf(u01(r.v[0]))), r1 = sqrtf(-2.0f * logf(u01(r.v[2])));
  float s0, c0, s1, c1;
  sincosf(6.283185307179586f * u01(r.v[1]), &s0, &c0);
  sincosf(6.283185307179586f * u01(r.v[3]), &s1, &c1);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}
constexpr unsigned OSM_RNG_STREAM_STEP_NOISE = 0x6f736d31u;   // "osm1": the per-step noise of a chain
__device__ __forceinline__ unsigned step_word(unsigned step, unsigned sub) { return step | (sub << 16); }

__global__ __launch_bounds__(256) void philox_raw_kernel(unsigned* __restrict__ out, long long n4, unsigned c1, unsigned c2,
                                                          unsigned c3, unsigned k0, unsigned k1) {
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (long long)gridDim.x * blockDim.x) {
    const Philox4 r = philox4x32_10((unsigned)q, c1, c2, c3, k0, k1);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[4 * q + e] = r.v[e];
  }
}

// out[b][0..n) ~ N(0, 1): image b uses counter word 1 = img0 + b, word 2 = the step (from the device counter when given) | sub << 16
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int B, long long n, unsigned k0, unsigned k1,
                                                     const int* __restrict__ step_dev, int step_const, unsigned sub, int img0,
                                                     int img_stride) {
  const unsigned step = step_word((unsigned)(step_dev ? *step_dev : step_const), sub);
  const long long nq = (n + 3) >> 2;
  const long long total = (long long)B * nq;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / nq, q = i - b * nq;
    float z[4];
    normal4(philox4x32_10((unsigned)q, (unsigned)(img0 + (int)b * img_stride), step, OSM_RNG_STREAM_STEP_NOISE, k0, k1), z);
    float* o = out + b * n + 4 * q;
    if (4 * q + 3 < n) *reinterpret_cast<float4*>(o) = make_float4(z[0], z[1], z[2], z[3]);    // (n % 4 == 0 and out 16-byte aligned: checked by the host)
    else for (int e = 0; e < 4 && 4 * q + e < n; ++e) o[e] = z[e];
  }
}

// guide_update with the noise drawn in the kernel: counter word 0 = element / 4 within the image's C HW elements (HW % 4 == 0: a
// quad never straddles two channels) -- osm_randn(_sub) with n = C HW draws the same
__global__ __launch_bounds__(256) void guide_update_rng_kernel(const float* __restrict__ mean, const float* __restrict__ logvar,
                                                                  const float* __restrict__ g, const float* __restrict__ dxu,
                                                                  const float* __restrict__ coef, const float* __restrict__ scale,
                                                                  float clip, float* __restrict__ x_next, float* __restrict__ grad_out,
                                                                  float* __restrict__ noise_out, int B, int C, int HW, unsigned k0,
                                                                  unsigned k1, const int* __restrict__ step_dev, int step_offset,
                                                                  unsigned sub, int img0, int img_stride) {
  const long long nq = (long long)C * (HW >> 2);
  const long long total = (long long)B * nq;
  const float c0 = coef[0], noise_on = coef[6];
  const unsigned step = step_word((unsigned)(*step_dev + step_offset), sub);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / nq, q = i - b * nq;
    const long long e0 = b * (long long)C * HW + 4 * q;
    const int c = (int)((4 * q) / HW);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (noise_on != 0.f) normal4(philox4x32_10((unsigned)q, (unsigned)(img0 + (int)b * img_stride), step, OSM_RNG_STREAM_STEP_NOISE, k0, k1), z);
    const float4 m = *reinterpret_cast<const float4*>(mean + e0);
    const float4 lv = *reinterpret_cast<const float4*>(logvar + e0);
    float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), du = gv;
    if (g) gv = *reinterpret_cast<const float4*>(g + e0);
    if (g && dxu) du = *reinterpret_cast<const float4*>(dxu + e0);
    const float mm[4] = {m.x, m.y, m.z, m.w}, ll[4] = {lv.x, lv.y, lv.z, lv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w},
                dd[4] = {du.x, du.y, du.z, du.w};
    float xo[4], go[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float grad = g ? c0 * gg[e] + dd[e] : 0.f;
      go[e] = grad;
      float gc = grad;
      if (clip >= 0.f) gc = (grad != grad) ? grad : fminf(fmaxf(grad, -clip), clip);
      float xt = mm[e] - (g ? scale[c] * gc : 0.f);
      if (noise_on != 0.f) xt += expf(0.5f * ll[e]) * z[e];
      xo[e] = xt;
    }
    *reinterpret_cast<float4*>(x_next + e0) = make_float4(xo[0], xo[1], xo[2], xo[3]);
    if (grad_out) *reinterpret_cast<float4*>(grad_out + e0) = make_float4(go[0], go[1], go[2], go[3]);
    if (noise_out) *reinterpret_cast<float4*>(noise_out + e0) = make_float4(z[0], z[1], z[2], z[3]);
  }
}

// ---------------------------------------------------------------- few-step solvers (include/osmosis_solver.h: DDIM, DPM-Solver++ 2M)
// x_next = A x + B0 x0 + B1 hist + S z - scale[c] clamp(grad), hist <- x0, with the four coefficients of the rule in srow
// (host, float64 -> fp32).  A lane owns four consecutive elements of the flat [B,C,HW] range: VEC (HW % 4 == 0, every pointer
// 16-byte aligned: one quad lies in one channel of one image) moves them as one 16-byte access per tensor, otherwise one by one.
// Every element is read (x, hist), then written (x_next, hist), by its one lane: x_next may alias x.

// One element, no contraction: every product and every sum is rounded once, in this order.  The gradient arrives formed.
__device__ __forceinline__ float solver_elem(float A, float B0, float B1, float S, bool noisy, float xv, float x0v, float hv, float zv,
                                             bool guided, float sc, float clip, float grad) {
#pragma clang fp contract(off)
  float t = A * xv;
  t += B0 * x0v;
  if (B1 != 0.f) t += B1 * hv;
  if (noisy) t += S * zv;
  if (!guided) return t;
  float gc = grad;
  if (clip >= 0.f) gc = (grad != grad) ? grad : fminf(fmaxf(grad, -clip), clip);   // torch.clamp keeps NaN
  return t - sc * gc;
}

struct SolverArgs {
  const float* x0; const float* x; float* hist; const float* g; const float* dxu; const float* noise; const float* coef;
  const float* srow; const float* scale; float clip; float* x_next; float* grad_out; float* noise_out; int B, C, HW;
};

// RNG: z is drawn here (counter words as guide_update_rng_kernel: element quad of the image, image, step | sub << 16, stream id)
// instead of read from a.noise; it requires VEC.
template <bool RNG, bool VEC>
__device__ __forceinline__ void solver_update_body(const SolverArgs& a, unsigned k0, unsigned k1, unsigned step, int img0, int img_stride) {
  static_assert(!RNG || VEC, "one Philox counter covers four consecutive elements of one channel");
  const long long total = (long long)a.B * a.C * a.HW;
  const long long nquad = (total + 3) >> 2;
  const long long nq = ((long long)a.C * a.HW) >> 2;       // (VEC: quads per image)
  const float c0 = a.coef[0];
  const float A = a.srow[0], B0 = a.srow[1], B1 = a.srow[2], S = a.srow[3];
  const bool noisy = S != 0.f && a.srow[4] != 0.f && (RNG || a.noise != nullptr);
  const bool guided = a.g != nullptr;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nquad; i += (long long)gridDim.x * blockDim.x) {
    const long long e0 = 4 * i;
    float xv[4], x0v[4], hv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f},
          dv[4] = {0.f, 0.f, 0.f, 0.f}, sc[4] = {0.f, 0.f, 0.f, 0.f}, xo[4], go[4];
    int n = 4;
    if constexpr (VEC) {
      const float4 vx = *reinterpret_cast<const float4*>(a.x + e0), v0 = *reinterpret_cast<const float4*>(a.x0 + e0);
      xv[0] = vx.x; xv[1] = vx.y; xv[2] = vx.z; xv[3] = vx.w;
      x0v[0] = v0.x; x0v[1] = v0.y; x0v[2] = v0.z; x0v[3] = v0.w;
      if (B1 != 0.f) {
        const float4 vh = *reinterpret_cast<const float4*>(a.hist + e0);
        hv[0] = vh.x; hv[1] = vh.y; hv[2] = vh.z; hv[3] = vh.w;
      }
      if (guided) {
        const float4 vg = *reinterpret_cast<const float4*>(a.g + e0);
        gv[0] = vg.x; gv[1] = vg.y; gv[2] = vg.z; gv[3] = vg.w;
        if (a.dxu) {
          const float4 vd = *reinterpret_cast<const float4*>(a.dxu + e0);
          dv[0] = vd.x; dv[1] = vd.y; dv[2] = vd.z; dv[3] = vd.w;
        }
        const float s = a.scale[(int)((e0 / a.HW) % a.C)];
        sc[0] = sc[1] = sc[2] = sc[3] = s;
      }
      if (noisy) {
        if constexpr (RNG) {
          const long long b = i / nq, q = i - b * nq;
          normal4(philox4x32_10((unsigned)q, (unsigned)(img0 + (int)b * img_stride), step, OSM_RNG_STREAM_STEP_NOISE, k0, k1), zv);
        } else {
          const float4 vz = *reinterpret_cast<const float4*>(a.noise + e0);
          zv[0] = vz.x; zv[1] = vz.y; zv[2] = vz.z; zv[3] = vz.w;
        }
      }
    } else {
      n = (int)(total - e0 < 4 ? total - e0 : 4);
      for (int e = 0; e < n; ++e) {
        const long long k = e0 + e;
        xv[e] = a.x[k]; x0v[e] = a.x0[k];
        if (B1 != 0.f) hv[e] = a.hist[k];
        if (guided) {
          gv[e] = a.g[k];
          if (a.dxu) dv[e] = a.dxu[k];
          sc[e] = a.scale[(int)((k / a.HW) % a.C)];
        }
        if (noisy) zv[e] = a.noise[k];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) {
        go[e] = guided ? fmaf(c0, gv[e], dv[e]) : 0.f;        // c0 g + dx_unet as guide_update forms it: one rounding
        xo[e] = solver_elem(A, B0, B1, S, noisy, xv[e], x0v[e], hv[e], zv[e], guided, sc[e], a.clip, go[e]);
      }
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(a.x_next + e0) = make_float4(xo[0], xo[1], xo[2], xo[3]);
      *reinterpret_cast<float4*>(a.hist + e0) = make_float4(x0v[0], x0v[1], x0v[2], x0v[3]);
      if (a.grad_out) *reinterpret_cast<float4*>(a.grad_out + e0) = make_float4(go[0], go[1], go[2], go[3]);
      if (a.noise_out) *reinterpret_cast<float4*>(a.noise_out + e0) = make_float4(zv[0], zv[1], zv[2], zv[3]);
    } else {
      for (int e = 0; e < n; ++e) {
        const long long k = e0 + e;
        a.x_next[k] = xo[e];
        a.hist[k] = x0v[e];
        if (a.grad_out) a.grad_out[k] = go[e];
        if (a.noise_out) a.noise_out[k] = zv[e];
      }
    }
  }
}

__global__ __launch_bounds__(256) void solver_update_kernel(SolverArgs a, int vec) {
  if (vec) solver_update_body<false, true>(a, 0u, 0u, 0u, 0, 0);
  else solver_update_body<false, false>(a, 0u, 0u, 0u, 0, 0);
}

__global__ __launch_bounds__(256) void solver_update_rng_kernel(SolverArgs a, unsigned k0, unsigned k1,
                                                                 const int* __restrict__ step_dev, int step_offset, unsigned sub,
                                                                 int img0, int img_stride) {
  solver_update_body<true, true>(a, k0, k1, step_word((unsigned)(*step_dev + step_offset), sub), img0, img_stride);
}

// DDIM step + guidance (gaussian_diffusion.py:505-535, condition_methods.py:247-251), in the reference's operation order:
//   eps = (r0 x - x0) / r1 ; sigma = eta sqrt((1 - abp) / (1 - ab)) sqrt(1 - ab / abp) ;
//   x_next = x0 sqrt(abp) + sqrt(1 - abp - sigma^2) eps + [t != 0] sigma noise - scale[c] clamp(grad) ; grad = c0 g + dx_unet
// coef = the posterior row (c0 = d x0 / d x of the mean processor), dcoef = {alpha_bar, alpha_bar_prev, eta, noise_on,
// r0 = sqrt_recip_ac, r1 = sqrt_recipm1_ac}: predict_eps_from_x_start (:533-536) uses the SAMPLER's tables whatever the mean
// processor is (for `epsilon` r0 = c0 and r1 = c1).
// x_next may alias x (each element is read, then written, by one thread)
__global__ __launch_bounds__(256) void ddim_update_kernel(const float* __restrict__ x0, const float* x, const float* __restrict__ g,
                                                             const float* __restrict__ dxu, const float* __restrict__ noise,
                                                             const float* __restrict__ coef, const float* __restrict__ dcoef,
                                                             const float* __restrict__ scale, float clip, float* x_next,
                                                             float* __restrict__ grad_out, int B, int C, int HW) {
  const long long total = (long long)B * C * HW;
  const float c0 = coef[0];
  const float ab = dcoef[0], abp = dcoef[1], eta = dcoef[2], noise_on = dcoef[3], r0 = dcoef[4], r1 = dcoef[5];
  const float sigma = eta * sqrtf((1.0f - abp) / (1.0f - ab)) * sqrtf(1.0f - ab / abp);
  const float sa = sqrtf(abp), sb = sqrtf(1.0f - abp - sigma * sigma);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)((i / HW) % C);
    const float xs = x0[i];
    const float eps = (r0 * x[i] - xs) / r1;
    float xt = xs * sa + sb * eps;
    if (noise_on != 0.f && noise) xt += sigma * noise[i];
    float grad = 0.f;
    if (g) grad = c0 * g[i] + (dxu ? dxu[i] : 0.f);
    if (grad_out) grad_out[i] = grad;
    float gc = grad;
    if (clip >= 0.f) gc = (grad != grad) ? grad : fminf(fmaxf(grad, -clip), clip);
    x_next[i] = xt - (g ? scale[c] * gc : 0.f);
  }
}

__global__ void fetch_coefs_kernel(const float* __restrict__ table, int* __restrict__ step, int delta,
                                   float* __restrict__ coef_out, float* __restrict__ t_out, int B, int n_rows) {
  const int s = min(max(*step, 0), n_rows - 1);   // a counter that ran off the table re-reads its last row
  if (threadIdx.x < 8) coef_out[threadIdx.x] = table[s * 8 + threadIdx.x];
  if (threadIdx.x < B) t_out[threadIdx.x] = table[s * 8 + 7];
  __syncthreads();
  if (threadIdx.x == 0) *step = s + delta;
}

inline int grid_for(long long total) {
  long long b = (total + 255) / 256;
  if (b > 2048) b = 2048;
  return (int)(b < 1 ? 1 : b);
}

int check_desc(const osm_phys_desc* d, const char* who) {
  OSM_REQUIRE(d, "%s: null descriptor", who);
  OSM_REQUIRE(d->kind >= 0 && d->kind <= 3, "%s: unknown operator kind %d", who, d->kind);
  OSM_REQUIRE(d->kind != 3 || (d->loss_type == 0 && d->weight_type == 0 && d->gamma_avrg == 0.f && d->gamma_val == 0.f),
              "%s: the identity operator (kind 3) is the plain norm loss: no weight, no auxiliary losses", who);
  OSM_REQUIRE(d->depth_type >= 0 && d->depth_type <= 2, "%s: unknown depth_type %d", who, d->depth_type);
  OSM_REQUIRE(d->loss_type == 0 || d->loss_type == 1, "%s: unknown loss_type %d", who, d->loss_type);
  OSM_REQUIRE(d->B > 0 && d->HW > 0, "%s: bad shape", who);
  return OSM_OK;
}

}  // namespace

extern "C" int osm_phys_nblk(int HW) { return (HW + PPB - 1) / PPB; }

namespace {
int check_lin_desc(const osm_phys_desc* d, const char* who) {
  int rc = check_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(d->kind != 3, "%s: the identity operator (kind 3) has no image-formation model to compose with", who);
  return OSM_OK;
}

// What a phi step needs.  The schedules ask before their first launch: a failure of a later finalize would leave phi half-stepped.
int check_phi_step(const char* who, const osm_phys_desc* d, int do_update, const float* opt_state, bool routed = false) {
  OSM_REQUIRE(d->optimizer >= 0 && d->optimizer <= 9, "%s: optimizer must be 0 (sgd / GD) .. 9 (see osm_phys_desc)", who);
  if (d->optimizer == 9) {
    OSM_REQUIRE(!routed, "%s: optimizer 9 (lm, the Levenberg-Marquardt phi solver) does not run on the composed (degradation) or "
                "grouped (phi_groups) routes", who);
    OSM_REQUIRE(d->kind != 3, "%s: optimizer 9 (lm) needs an image-formation model: the identity operator (kind 3) has no parameters", who);
    OSM_REQUIRE(do_update >= 0 && do_update <= 3, "%s: optimizer 9 (lm) takes do_update 0 (loss only), 1 (step), 2 (first step of a call) "
                "or 3 (close), got %d", who, do_update);
  }
  OSM_REQUIRE(!(d->optimizer != 0 && do_update) || opt_state, "%s: a stateful optimizer needs opt_state [B][20]", who);
  OSM_REQUIRE(!(d->kind == 3 && do_update), "%s: the identity operator (kind 3) has no parameters to step", who);
  return OSM_OK;
}

// The composed route's arguments (include/osmosis_physlin.h): the measurement's size, v = A^T u and the residual's partial sums.  A
// launcher that is handed one runs its kernel's LIN instantiation; each checks the members it reads.
struct LinArgs { int hw; const float* v; const float* part_r; };

int phys_reduce_launch(const char* who, const osm_phys_desc* d, const float* x0, const float* y, const float* mask, const float* phi,
                       float* part, void* stream, const LinArgs* la = nullptr, bool plain = false) {
  int rc = la ? check_lin_desc(d, who) : check_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(x0 && phi && part && (la ? la->v != nullptr : y != nullptr), "%s: null pointer", who);
  const int nblk = osm_phys_nblk(d->HW);
  const dim3 grid(nblk, d->B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (d->optimizer == 9 && !plain) {      // the LM solver's reduce: 32 floats per workgroup (`plain`: its schedule's closing evaluation)
    if ((rc = check_phi_step(who, d, 0, nullptr, la != nullptr))) return rc;
    if (mask) hipLaunchKernelGGL(phys_lm_reduce_kernel<true>, grid, block, 0, st, *d, x0, y, mask, phi, part, nblk);
    else hipLaunchKernelGGL(phys_lm_reduce_kernel<false>, grid, block, 0, st, *d, x0, y, nullptr, phi, part, nblk);
    return osm::check_launch("phys_lm_reduce_kernel");
  }
  if (la) hipLaunchKernelGGL((phys_reduce_kernel<false, true>), grid, block, 0, st, *d, x0, nullptr, nullptr, phi, la->v, part, nblk);
  else if (mask) hipLaunchKernelGGL((phys_reduce_kernel<true, false>), grid, block, 0, st, *d, x0, y, mask, phi, nullptr, part, nblk);
  else hipLaunchKernelGGL((phys_reduce_kernel<false, false>), grid, block, 0, st, *d, x0, y, nullptr, phi, nullptr, part, nblk);
  return osm::check_launch("phys_reduce_kernel");
}

// The offsets of a group descriptor, validated and copied by value (they travel in the kernel's arguments).
int check_group(const osm_phys_desc* d, const osm_group_desc* grp, GroupOff* go, const char* who) {
  OSM_REQUIRE(grp, "%s: null group descriptor", who);
  OSM_REQUIRE(grp->G >= 1 && grp->G <= OSM_MAX_GROUPS, "%s: G = %d groups, must be 1 .. %d", who, grp->G, OSM_MAX_GROUPS);
  OSM_REQUIRE(grp->off, "%s: null pointer (group offsets)", who);
  OSM_REQUIRE(grp->reduce == 0 || grp->reduce == 1, "%s: reduce must be 0 (sum) or 1 (mean), got %d", who, grp->reduce);
  OSM_REQUIRE(grp->off[0] == 0, "%s: off[0] must be 0, got %d", who, grp->off[0]);
  for (int j = 0; j < grp->G; ++j)
    OSM_REQUIRE(grp->off[j + 1] > grp->off[j], "%s: group offsets must be strictly increasing (off[%d] = %d, off[%d] = %d)", who, j,
                grp->off[j], j + 1, grp->off[j + 1]);
  OSM_REQUIRE(grp->off[grp->G] == d->B, "%s: off[G] = %d must be the batch B = %d", who, grp->off[grp->G], d->B);
  for (int j = 0; j <= grp->G; ++j) go->off[j] = grp->off[j];
  go->G = grp->G;
  go->reduce_mean = grp->reduce;
  return OSM_OK;
}

// go == nullptr: the per-image finalize; else one phi step per group
int phys_finalize_launch(const char* who, const osm_phys_desc* d, const float* part, float* red, float* phi, int do_update,
                         float* loss_out, float* opt_state, int zero_guard, void* stream, const GroupOff* go = nullptr,
                         const LinArgs* la = nullptr) {
  int rc = la ? check_lin_desc(d, who) : check_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(!la || (la->hw >= 1 && la->hw < (1 << 29)), "%s: bad measurement size hw = %d", who, la->hw);
  OSM_REQUIRE(part && red && phi && (!la || la->part_r), "%s: null pointer", who);
  if ((rc = check_phi_step(who, d, do_update, opt_state, go || la))) return rc;
  const int nblk = osm_phys_nblk(d->HW);
  const dim3 grid(go ? go->G : d->B), block(go ? 64 * GWAVES : 64);
  hipStream_t st = (hipStream_t)stream;
  if (d->optimizer == 9 && do_update) {   // the LM solver decides (and steps); do_update = 0 is the plain finalize below
    hipLaunchKernelGGL(phys_lm_finalize_kernel, grid, block, 0, st, *d, part, red, phi, do_update, loss_out, opt_state, nblk);
    return osm::check_launch("phys_lm_finalize_kernel");
  }
  if (go && la) {
    hipLaunchKernelGGL(phys_finalize_group_kernel<true>, grid, block, 0, st, *d, part, red, phi, do_update, loss_out, opt_state, nblk,
                       zero_guard, *go, FinLin<true>{la->part_r, osm_phys_nblk(la->hw), la->hw});
  } else if (go) {
    hipLaunchKernelGGL(phys_finalize_group_kernel<false>, grid, block, 0, st, *d, part, red, phi, do_update, loss_out, opt_state, nblk,
                       zero_guard, *go, FinLin<false>{});
  } else if (la) {
    hipLaunchKernelGGL(phys_finalize_kernel<true>, grid, block, 0, st, *d, part, red, phi, do_update, loss_out, opt_state, nblk,
                       zero_guard, FinLin<true>{la->part_r, osm_phys_nblk(la->hw), la->hw});
  } else {
    hipLaunchKernelGGL(phys_finalize_kernel<false>, grid, block, 0, st, *d, part, red, phi, do_update, loss_out, opt_state, nblk,
                       zero_guard, FinLin<false>{});
  }
  return osm::check_launch("phys_finalize_kernel");
}

int phys_grad_launch(const char* who, const osm_phys_desc* d, const float* x0, const float* y, const float* mask, const float* phi,
                     const float* red, float* g, void* stream, const LinArgs* la = nullptr, int zero_guard = 0) {
  int rc = la ? check_lin_desc(d, who) : check_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(!la || (la->hw >= 1 && la->hw < (1 << 29)), "%s: bad measurement size hw = %d", who, la->hw);
  OSM_REQUIRE(x0 && phi && red && g && (la ? la->v != nullptr : y != nullptr), "%s: null pointer", who);
  const dim3 grid((d->HW + 255) / 256, d->B), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (la) {
    hipLaunchKernelGGL((phys_grad_kernel<false, true>), grid, block, 0, st, *d, x0, nullptr, nullptr, phi, la->v, red, g, la->hw,
                       zero_guard);
  } else if (mask) {
    hipLaunchKernelGGL((phys_grad_kernel<true, false>), grid, block, 0, st, *d, x0, y, mask, phi, nullptr, red, g, 0, 0);
  } else {
    hipLaunchKernelGGL((phys_grad_kernel<false, false>), grid, block, 0, st, *d, x0, y, nullptr, phi, nullptr, red, g, 0, 0);
  }
  return osm::check_launch("phys_grad_kernel");
}

int check_lin(const osm_phys_desc* d, const osm_lin_desc* l, const char* who) {
  OSM_REQUIRE(l, "%s: null operator descriptor", who);
  OSM_REQUIRE(l->family == 0 || l->family == 1, "%s: unknown operator family %d (0 separable, 1 psf)", who, l->family);
  OSM_REQUIRE(l->H >= 1 && l->W >= 1 && l->h >= 1 && l->w >= 1, "%s: bad operator grids %d x %d -> %d x %d", who, l->H, l->W, l->h, l->w);
  OSM_REQUIRE((long long)l->H * l->W == (long long)d->HW, "%s: the operator's image grid %d x %d does not have the descriptor's HW = %d pixels",
              who, l->H, l->W, d->HW);
  OSM_REQUIRE((long long)l->h * l->w < (1LL << 29), "%s: measurement grid %d x %d too large", who, l->h, l->w);
  if (l->family == 0) {
    OSM_REQUIRE(l->start_h && l->wt_h && l->start_w && l->wt_w && l->tstart_h && l->twt_h && l->tstart_w && l->twt_w,
                "%s: a separable operator needs its forward and transposed band tables", who);
    OSM_REQUIRE(l->Kh >= 1 && l->Kw >= 1 && l->tKh >= 1 && l->tKw >= 1, "%s: bad band widths Kh %d, Kw %d, tKh %d, tKw %d", who, l->Kh, l->Kw,
                l->tKh, l->tKw);
  } else {
    OSM_REQUIRE(l->h == l->H && l->w == l->W, "%s: a psf operator keeps the image's grid, got %d x %d -> %d x %d", who, l->H, l->W, l->h, l->w);
    OSM_REQUIRE(l->dy && l->dx && l->tap_w, "%s: a psf operator needs its tap list", who);
    OSM_REQUIRE(l->T >= 1, "%s: bad tap count T %d", who, l->T);
    OSM_REQUIRE(l->Ry >= 0 && l->Rx >= 0 && l->Ry < l->H && l->Rx < l->W, "%s: reflection padding needs the radius 0 <= Ry %d < H %d and 0 <= Rx %d < W %d",
                who, l->Ry, l->H, l->Rx, l->W);
  }
  return OSM_OK;
}

inline int lin_planes(const osm_phys_desc* d) { return d->weight_type == 1 ? 4 : 3; }

// out [B,P,h w] = A x [B,P,H W] (adjoint = 0) or out [B,P,H W] = A^T x [B,P,h w] (adjoint = 1), P planes, densely packed images
int lin_apply(const osm_lin_desc* l, const float* x, float* out, int B, int P, int adjoint, void* stream) {
  const long long HW = (long long)l->H * l->W, hw = (long long)l->h * l->w;
  if (l->family == 1) return osm_psf_apply(x, out, l->dy, l->dx, l->tap_w, l->T, l->Ry, l->Rx, B, P, P * HW, P * HW, l->H, l->W, adjoint, 0, stream);
  if (adjoint)
    return osm_linop_apply(x, out, l->tstart_h, l->twt_h, l->tstart_w, l->twt_w, B, P, P * hw, P * HW, l->h, l->w, l->H, l->W, l->tKh,
                           l->tKw, 0, stream);
  return osm_linop_apply(x, out, l->start_h, l->wt_h, l->start_w, l->wt_w, B, P, P * HW, P * hw, l->H, l->W, l->h, l->w, l->Kh, l->Kw, 0,
                         stream);
}
}  // namespace

extern "C" int osm_phys_reduce(const osm_phys_desc* d, const float* x0, const float* y, const float* phi,
                               float* part, void* stream) {
  return phys_reduce_launch("osm_phys_reduce", d, x0, y, nullptr, phi, part, stream);
}

extern "C" int osm_phys_finalize(const osm_phys_desc* d, const float* part, float* red, float* phi,
                                 int do_update, float* loss_out, float* opt_state, void* stream) {
  return phys_finalize_launch("osm_phys_finalize", d, part, red, phi, do_update, loss_out, opt_state, 0, stream);
}

extern "C" int osm_phys_grad(const osm_phys_desc* d, const float* x0, const float* y, const float* phi,
                             const float* red, float* g, void* stream) {
  return phys_grad_launch("osm_phys_grad", d, x0, y, nullptr, phi, red, g, stream);
}

// The masked entry points (`_m`): mask [B,3,HW] in [0, 1], laid out like y; mask == NULL is the plain entry point, launch for launch.
extern "C" int osm_phys_reduce_m(const osm_phys_desc* d, const float* x0, const float* y, const float* mask, const float* phi,
                                 float* part, void* stream) {
  return phys_reduce_launch("osm_phys_reduce_m", d, x0, y, mask, phi, part, stream);
}

extern "C" int osm_phys_finalize_m(const osm_phys_desc* d, const float* part, float* red, float* phi, int do_update,
                                   float* loss_out, float* opt_state, int masked, void* stream) {
  return phys_finalize_launch("osm_phys_finalize_m", d, part, red, phi, do_update, loss_out, opt_state, masked != 0, stream);
}

extern "C" int osm_phys_grad_m(const osm_phys_desc* d, const float* x0, const float* y, const float* mask, const float* phi,
                               const float* red, float* g, void* stream) {
  return phys_grad_launch("osm_phys_grad_m", d, x0, y, mask, phi, red, g, stream);
}

// ---------------------------------------------------------------- the composed data term (include/osmosis_physlin.h)
extern "C" int osm_phys_forward(const osm_phys_desc* d, const float* x0, const float* phi, float* F, void* stream) {
  const char* who = "osm_phys_forward";
  int rc = check_lin_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(x0 && phi && F, "%s: null pointer", who);
  hipLaunchKernelGGL(phys_forward_kernel, dim3((d->HW + 255) / 256, d->B), dim3(256), 0, (hipStream_t)stream, *d, x0, phi, F,
                     lin_planes(d));
  return osm::check_launch("phys_forward_kernel");
}

extern "C" int osm_phys_resid(const osm_phys_desc* d, int hw, const float* AF, const float* y, const float* mask, float* u,
                              float* part_r, void* stream) {
  const char* who = "osm_phys_resid";
  int rc = check_lin_desc(d, who);
  if (rc) return rc;
  OSM_REQUIRE(hw >= 1 && hw < (1 << 29), "%s: bad measurement size hw = %d", who, hw);
  OSM_REQUIRE(AF && y && u && part_r, "%s: null pointer", who);
  const int nblk = osm_phys_nblk(hw);
  hipLaunchKernelGGL(phys_resid_kernel, dim3(nblk, d->B), dim3(256), 0, (hipStream_t)stream, AF, y, mask, u, part_r, lin_planes(d), hw,
                     nblk);
  return osm::check_launch("phys_resid_kernel");
}

extern "C" int osm_phys_reduce_lin(const osm_phys_desc* d, const float* x0, const float* phi, const float* v, float* part,
                                   void* stream) {
  const LinArgs la{0, v, nullptr};
  return phys_reduce_launch("osm_phys_reduce_lin", d, x0, nullptr, nullptr, phi, part, stream, &la);
}

extern "C" int osm_phys_finalize_lin(const osm_phys_desc* d, int hw, const float* part, const float* part_r, float* red, float* phi,
                                     int do_update, float* loss_out, float* opt_state, int masked, void* stream) {
  const LinArgs la{hw, nullptr, part_r};
  return phys_finalize_launch("osm_phys_finalize_lin", d, part, red, phi, do_update, loss_out, opt_state, masked != 0, stream, nullptr,
                              &la);
}

extern "C" int osm_phys_grad_lin(const osm_phys_desc* d, int hw, const float* x0, const float* phi, const float* v, const float* red,
                                 float* g, int masked, void* stream) {
  const LinArgs la{hw, v, nullptr};
  return phys_grad_launch("osm_phys_grad_lin", d, x0, nullptr, nullptr, phi, red, g, stream, &la, masked != 0);
}

// ---------------------------------------------------------------- the inner loop of one guided step, enqueued by ONE call
namespace {
// The composed route's operator and workspaces; a null pointer to one is the plain route.
struct LinWs { const osm_lin_desc* lin; float *F, *AF, *u, *v, *part_r; };

// The inner phi optimisation + dL/dx0 (measurements.py:266-303, condition_methods.py:109-144):
//   n_inner x { reduce; finalize (+ phi step) }, with the loss and the x0-gradient taken at the phi of the LAST iteration, which is
//   stepped afterwards (unless freeze_phi: then n_inner = 1 and phi stays).  The composed route runs forward, A, resid, A^T in front
//   of every reduce; `go` puts the grouped finalize in the place of the per-image one.  The same launches as the single entry points
//   in the same order -- from C the 2 n_inner + 2 launches cost the host ~2 us each instead of a Python call each (measured: the GPU
//   idled 0.24 ms per step between them).  Every argument is checked before the first launch.
int phys_optimize_launch(const char* who, const osm_phys_desc* d, const float* x0, const float* y, const float* mask, float* phi,
                         float* part, float* red, float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state,
                         void* stream, const GroupOff* go = nullptr, const LinWs* lw = nullptr) {
  int rc = lw ? check_lin_desc(d, who) : check_desc(d, who);
  if (rc) return rc;
  if (lw && (rc = check_lin(d, lw->lin, who))) return rc;
  OSM_REQUIRE(x0 && y && phi && part && red && loss_out && g && (!lw || (lw->F && lw->AF && lw->u && lw->v && lw->part_r)),
              "%s: null pointer", who);
  OSM_REQUIRE(n_inner >= 1, "%s: n_inner must be >= 1", who);
  OSM_REQUIRE(!(freeze_phi && n_inner != 1), "%s: freeze_phi goes with n_inner = 1", who);
  if ((rc = check_phi_step(who, d, !freeze_phi, opt_state, go || lw))) return rc;
  OSM_REQUIRE(!lw || (long long)d->B * 4 <= 65535, "%s: batch %d is too large for one launch of the operator", who, d->B);
  const int zg = mask != nullptr, hw = lw ? lw->lin->h * lw->lin->w : 0, P = lin_planes(d);
  const LinArgs la_{hw, lw ? lw->v : nullptr, lw ? lw->part_r : nullptr}, *la = lw ? &la_ : nullptr;
  const bool lm = d->optimizer == 9;
  if (lm && !freeze_phi) {
    // The LM schedule: n_inner x { LM reduce; LM finalize that decides and steps }, then a closing evaluation -- the plain reduce at
    // the trial phi and the LM finalize in close mode, which on a reject puts phi_base back and writes red[0] = S_base (slots 10..13
    // depend on x0 only) -- so the loss and g are taken at an accepted phi.  2 n_inner + 3 launches.
    for (int it = 0; it < n_inner; ++it) {
      if ((rc = phys_reduce_launch(who, d, x0, y, mask, phi, part, stream))) return rc;
      if ((rc = phys_finalize_launch(who, d, part, red, phi, it == 0 ? 2 : 1, loss_out, opt_state, zg, stream))) return rc;
    }
    if ((rc = phys_reduce_launch(who, d, x0, y, mask, phi, part, stream, nullptr, true))) return rc;
    if ((rc = phys_finalize_launch(who, d, part, red, phi, 3, loss_out, opt_state, zg, stream))) return rc;
    return phys_grad_launch(who, d, x0, y, mask, phi, red, g, stream, nullptr, zg);
  }
  for (int it = 0; it < n_inner; ++it) {
    if (lw) {
      if ((rc = osm_phys_forward(d, x0, phi, lw->F, stream))) return rc;
      if ((rc = lin_apply(lw->lin, lw->F, lw->AF, d->B, P, 0, stream))) return rc;
      if ((rc = osm_phys_resid(d, hw, lw->AF, y, mask, lw->u, lw->part_r, stream))) return rc;
      if ((rc = lin_apply(lw->lin, lw->u, lw->v, d->B, 3, 1, stream))) return rc;
    }
    if ((rc = phys_reduce_launch(who, d, x0, y, mask, phi, part, stream, la, lm))) return rc;   // (lm here: freeze_phi)
    if (it < n_inner - 1) {
      if ((rc = phys_finalize_launch(who, d, part, red, phi, 1, loss_out, opt_state, zg, stream, go, la))) return rc;
      continue;
    }
    if ((rc = phys_finalize_launch(who, d, part, red, phi, 0, loss_out, nullptr, zg, stream, go, la))) return rc;
    if ((rc = phys_grad_launch(who, d, x0, y, mask, phi, red, g, stream, la, zg))) return rc;
    if (!freeze_phi && (rc = phys_finalize_launch(who, d, part, red, phi, 1, nullptr, opt_state, zg, stream, go, la))) return rc;
  }
  return OSM_OK;
}
}  // namespace

extern "C" int osm_phys_optimize(const osm_phys_desc* d, const float* x0, const float* y, float* phi, float* part, float* red,
                                 float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state, void* stream) {
  return phys_optimize_launch("osm_phys_optimize", d, x0, y, nullptr, phi, part, red, loss_out, g, n_inner, freeze_phi, opt_state,
                              stream);
}

extern "C" int osm_phys_optimize_m(const osm_phys_desc* d, const float* x0, const float* y, const float* mask, float* phi, float* part,
                                   float* red, float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state,
                                   void* stream) {
  return phys_optimize_launch("osm_phys_optimize_m", d, x0, y, mask, phi, part, red, loss_out, g, n_inner, freeze_phi, opt_state,
                              stream);
}

extern "C" int osm_phys_optimize_lin(const osm_phys_desc* d, const osm_lin_desc* lin, const float* x0, const float* y, const float* mask,
                                     float* phi, float* F, float* AF, float* u, float* v, float* part_r, float* part, float* red,
                                     float* loss_out, float* g, int n_inner, int freeze_phi, float* opt_state, void* stream) {
  const LinWs lw{lin, F, AF, u, v, part_r};
  return phys_optimize_launch("osm_phys_optimize_lin", d, x0, y, mask, phi, part, red, loss_out, g, n_inner, freeze_phi, opt_state,
                              stream, nullptr, &lw);
}

// ---------------------------------------------------------------- shared water parameters (include/osmosis_physgroup.h)
extern "C" int osm_phys_finalize_g(const osm_phys_desc* d, const osm_group_desc* grp, const float* part, float* red, float* phi,
                                   int do_update, float* loss_out, float* opt_state, int masked, void* stream) {
  const char* who = "osm_phys_finalize_g";
  GroupOff go;
  int rc = check_desc(d, who);
  if (rc) return rc;
  if ((rc = check_group(d, grp, &go, who))) return rc;
  return phys_finalize_launch(who, d, part, red, phi, do_update, loss_out, opt_state, masked != 0, stream, &go);
}

extern "C" int osm_phys_finalize_lin_g(const osm_phys_desc* d, const osm_group_desc* grp, int hw, const float* part, const float* part_r,
                                       float* red, float* phi, int do_update, float* loss_out, float* opt_state, int masked,
                                       void* stream) {
  const char* who = "osm_phys_finalize_lin_g";
  GroupOff go;
  int rc = check_lin_desc(d, who);
  if (rc) return rc;
  if ((rc = check_group(d, grp, &go, who))) return rc;
  const LinArgs la{hw, nullptr, part_r};
  return phys_finalize_launch(who, d, part, red, phi, do_update, loss_out, opt_state, masked != 0, stream, &go, &la);
}

extern "C" int osm_phys_optimize_g(const osm_phys_desc* d, const osm_group_desc* grp, const float* x0, const float* y, const float* mask,
                                   float* phi, float* part, float* red, float* loss_out, float* g, int n_inner, int freeze_phi,
                                   float* opt_state, void* stream) {
  const char* who = "osm_phys_optimize_g";
  GroupOff go;
  int rc = check_desc(d, who);
  if (rc) return rc;
  if ((rc = check_group(d, grp, &go, who))) return rc;
  return phys_optimize_launch(who, d, x0, y, mask, phi, part, red, loss_out, g, n_inner, freeze_phi, opt_state, stream, &go);
}

extern "C" int osm_phys_optimize_lin_g(const osm_phys_desc* d, const osm_group_desc* grp, const osm_lin_desc* lin, const float* x0,
                                       const float* y, const float* mask, float* phi, float* F, float* AF, float* u, float* v,
                                       float* part_r, float* part, float* red, float* loss_out, float* g, int n_inner, int freeze_phi,
                                       float* opt_state, void* stream) {
  const char* who = "osm_phys_optimize_lin_g";
  GroupOff go;
  int rc = check_lin_desc(d, who);
  if (rc) return rc;
  if ((rc = check_group(d, grp, &go, who))) return rc;
  const LinWs lw{lin, F, AF, u, v, part_r};
  return phys_optimize_launch(who, d, x0, y, mask, phi, part, red, loss_out, g, n_inner, freeze_phi, opt_state, stream, &go, &lw);
}

// ---------------------------------------------------------------- the step kernels' entry points
// The fixed-shape entry points are the channel-generic ones (`_c`) at (C, Cout) = (4, 8): one launch helper per kernel, which takes
// its caller's name for the messages.
namespace {
int check_kinds(const char* name, int mean_kind, int var_kind) {
  OSM_REQUIRE(mean_kind >= 0 && mean_kind <= 2, "%s: mean_kind must be 0 (epsilon), 1 (start_x) or 2 (previous_x)", name);
  OSM_REQUIRE(var_kind >= 0 && var_kind <= 2, "%s: var_kind must be 0 (learned_range), 1 (fixed) or 2 (learned)", name);
  return OSM_OK;
}

int check_cout(const char* name, int C, int Cout) {
  OSM_REQUIRE(C > 0 && (Cout == C || Cout == 2 * C), "%s: Cout must be C or 2 C, got C = %d, Cout = %d", name, C, Cout);
  return OSM_OK;
}

// (mean_kind and var_kind in range: check_kinds)
int posterior_launch(bool raw, const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind, float* x0_raw,
                     float* x0, float* mean, float* logvar, int B, int C, int Cout, int HW, hipStream_t st) {
  const dim3 grid(grid_for((long long)B * C * HW)), block(256);
#define OSM_POST1(MK, VK, RAW) \
  hipLaunchKernelGGL((posterior_kernel<MK, VK, RAW>), grid, block, 0, st, model_out, x, coef, x0_raw, x0, mean, logvar, B, C, Cout, HW)
#define OSM_POST(MK, VK) do { if (raw) OSM_POST1(MK, VK, true); else OSM_POST1(MK, VK, false); } while (0)
  switch (mean_kind * 3 + var_kind) {
    case 0: OSM_POST(0, 0); break;
    case 1: OSM_POST(0, 1); break;
    case 2: OSM_POST(0, 2); break;
    case 3: OSM_POST(1, 0); break;
    case 4: OSM_POST(1, 1); break;
    case 5: OSM_POST(1, 2); break;
    case 6: OSM_POST(2, 0); break;
    case 7: OSM_POST(2, 1); break;
    default: OSM_POST(2, 2); break;
  }
#undef OSM_POST
#undef OSM_POST1
  return osm::check_launch("posterior_kernel");
}

// dynamic_threshold: the raw pass, the batch-wide quantile of |x0_raw|, then x0 and the mean
int posterior_dynthr_launch(const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind, float s,
                            float* x0_raw, float* x0, float* mean, float* logvar, float* q, int* idx, void* ws, int B, int C, int Cout,
                            int HW, void* stream) {
  const long long total = (long long)B * C * HW;
  hipStream_t st = (hipStream_t)stream;
  int rc = posterior_launch(true, model_out, x, coef, mean_kind, var_kind, x0_raw, x0, mean, logvar, B, C, Cout, HW, st);
  if (rc) return rc;
  if ((rc = osm_quantile_abs(x0_raw, total, s, q, idx, ws, stream))) return rc;
  const dim3 grid(grid_for(total)), block(256);
  if (mean_kind == 2) {
    hipLaunchKernelGGL(dynthr_apply_kernel<2>, grid, block, 0, st, x0_raw, x, coef, q, x0, mean, total);
  } else {
    hipLaunchKernelGGL(dynthr_apply_kernel<0>, grid, block, 0, st, x0_raw, x, coef, q, x0, mean, total);
  }
  return osm::check_launch("dynthr_apply_kernel");
}

int posterior_bwd_launch(const char* name, const float* g, const float* coef, float* d_out, int B, int C, int Cout, int HW,
                         void* stream) {
  OSM_REQUIRE(g && coef && d_out && B > 0 && HW > 0, "%s: bad argument", name);
  int rc = check_cout(name, C, Cout);
  if (rc) return rc;
  hipLaunchKernelGGL(posterior_bwd_kernel, dim3(grid_for((long long)B * Cout * HW)), dim3(256), 0, (hipStream_t)stream, g, coef,
                     d_out, B, C, Cout, HW);
  return osm::check_launch("posterior_bwd_kernel");
}

int guide_update_launch(const char* name, const float* mean, const float* logvar, const float* g, const float* dx_unet,
                        const float* noise, const float* coef, const float* scale, float clip, float* x_next, float* grad_out, int B,
                        int C, int HW, void* stream) {
  OSM_REQUIRE(mean && logvar && coef && x_next && B > 0 && C > 0 && HW > 0, "%s: bad argument", name);
  OSM_REQUIRE(!g || scale, "%s: guidance needs the per-channel scale", name);
  hipLaunchKernelGGL(guide_update_kernel, dim3(grid_for((long long)B * C * HW)), dim3(256), 0, (hipStream_t)stream, mean, logvar,
                     g, dx_unet, noise, coef, scale, clip, x_next, grad_out, B, C, HW);
  return osm::check_launch("guide_update_kernel");
}

int guide_update_rng_launch(const char* name, const float* mean, const float* logvar, const float* g, const float* dx_unet,
                            const float* coef, const float* scale, float clip, float* x_next, float* grad_out, float* noise_out,
                            int B, int C, int HW, unsigned long long seed, const int* step, int step_offset, int sub, int img0,
                            int img_stride, void* stream) {
  OSM_REQUIRE(mean && logvar && coef && x_next && step && B > 0 && C > 0 && HW > 0, "%s: bad argument", name);
  OSM_REQUIRE(!g || scale, "%s: guidance needs the per-channel scale", name);
  OSM_REQUIRE(sub >= 0 && sub < 65536, "%s: sub must be in [0, 65536), got %d", name, sub);
  OSM_REQUIRE(HW % 4 == 0, "%s: H*W must be a multiple of 4 (one Philox counter per four elements of one channel)", name);
  OSM_REQUIRE(((reinterpret_cast<size_t>(mean) | reinterpret_cast<size_t>(logvar) | reinterpret_cast<size_t>(g) |
                reinterpret_cast<size_t>(dx_unet) | reinterpret_cast<size_t>(x_next) | reinterpret_cast<size_t>(grad_out) |
                reinterpret_cast<size_t>(noise_out)) & 15) == 0, "%s: tensors must be 16-byte aligned", name);
  hipLaunchKernelGGL(guide_update_rng_kernel, dim3(grid_for((long long)B * C * (HW / 4))), dim3(256), 0, (hipStream_t)stream, mean,
                     logvar, g, dx_unet, coef, scale, clip, x_next, grad_out, noise_out, B, C, HW, (unsigned)(seed & 0xffffffffull),
                     (unsigned)(seed >> 32), step, step_offset, (unsigned)sub, img0, img_stride);
  return osm::check_launch("guide_update_rng_kernel");
}

int ddim_update_launch(const char* name, const float* x0, const float* x, const float* g, const float* dx_unet, const float* noise,
                       const float* coef, const float* dcoef, const float* scale, float clip, float* x_next, float* grad_out, int B,
                       int C, int HW, void* stream) {
  OSM_REQUIRE(x0 && x && coef && dcoef && x_next && B > 0 && C > 0 && HW > 0, "%s: bad argument", name);
  OSM_REQUIRE(!g || scale, "%s: guidance needs the per-channel scale", name);
  hipLaunchKernelGGL(ddim_update_kernel, dim3(grid_for((long long)B * C * HW)), dim3(256), 0, (hipStream_t)stream, x0, x, g,
                     dx_unet, noise, coef, dcoef, scale, clip, x_next, grad_out, B, C, HW);
  return osm::check_launch("ddim_update_kernel");
}

// The argument checks of include/osmosis_solver.h, before any launch; *vec: whether every tensor can move as 16-byte quads.
int solver_check(const char* name, const SolverArgs& a, int* vec) {
  OSM_REQUIRE(a.x0 && a.x && a.hist && a.coef && a.srow && a.x_next, "%s: x0, x, hist, coef, srow and x_next must be given", name);
  OSM_REQUIRE(a.B > 0 && a.C > 0 && a.HW > 0, "%s: bad shape B %d, C %d, HW %d", name, a.B, a.C, a.HW);
  OSM_REQUIRE(!a.g || a.scale, "%s: guidance needs the per-channel scale", name);
  OSM_REQUIRE(a.g || !a.dxu, "%s: dx_unet without g", name);
  OSM_REQUIRE(a.clip == a.clip, "%s: clip is NaN (negative: no clamp)", name);
  OSM_REQUIRE(a.hist != a.x0 && a.hist != a.x && a.hist != a.x_next, "%s: hist must be a buffer of its own", name);
  const size_t bits = reinterpret_cast<size_t>(a.x0) | reinterpret_cast<size_t>(a.x) | reinterpret_cast<size_t>(a.hist) |
                      reinterpret_cast<size_t>(a.g) | reinterpret_cast<size_t>(a.dxu) | reinterpret_cast<size_t>(a.noise) |
                      reinterpret_cast<size_t>(a.x_next) | reinterpret_cast<size_t>(a.grad_out) | reinterpret_cast<size_t>(a.noise_out);
  *vec = a.HW % 4 == 0 && (bits & 15) == 0;
  return OSM_OK;
}

int solver_update_launch(const char* name, const SolverArgs& a, void* stream) {
  int vec = 0;
  const int rc = solver_check(name, a, &vec);
  if (rc != OSM_OK) return rc;
  const long long nquad = ((long long)a.B * a.C * a.HW + 3) / 4;
  hipLaunchKernelGGL(solver_update_kernel, dim3(grid_for(nquad)), dim3(256), 0, (hipStream_t)stream, a, vec);
  return osm::check_launch("solver_update_kernel");
}

int solver_update_rng_launch(const char* name, const SolverArgs& a, unsigned long long seed, const int* step, int step_offset, int sub,
                             int img0, int img_stride, void* stream) {
  int vec = 0;
  const int rc = solver_check(name, a, &vec);
  if (rc != OSM_OK) return rc;
  OSM_REQUIRE(step, "%s: the device step counter must be given", name);
  OSM_REQUIRE(sub >= 0 && sub < 65536, "%s: sub must be in [0, 65536), got %d", name, sub);
  OSM_REQUIRE(a.HW % 4 == 0, "%s: H*W must be a multiple of 4 (one Philox counter per four elements of one channel)", name);
  OSM_REQUIRE(vec, "%s: tensors must be 16-byte aligned", name);
  const long long nquad = (long long)a.B * a.C * (a.HW / 4);
  hipLaunchKernelGGL(solver_update_rng_kernel, dim3(grid_for(nquad)), dim3(256), 0, (hipStream_t)stream, a,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), step, step_offset, (unsigned)sub, img0, img_stride);
  return osm::check_launch("solver_update_rng_kernel");
}

int randn_launch(const char* name, float* out, int B, long long n, unsigned long long seed, const int* step_dev, int step_const,
                 int sub, int img0, int img_stride, void* stream) {
  OSM_REQUIRE(out && B > 0 && n > 0, "%s: bad argument", name);
  OSM_REQUIRE(sub >= 0 && sub < 65536, "%s: sub must be in [0, 65536), got %d", name, sub);
  OSM_REQUIRE(sub == 0 || step_dev || (step_const >= 0 && step_const < 65536),
              "%s: with sub != 0 the step must be in [0, 65536), got %d", name, step_const);
  OSM_REQUIRE((reinterpret_cast<size_t>(out) & 15) == 0, "%s: out must be 16-byte aligned", name);
  OSM_REQUIRE(n % 4 == 0 || B == 1, "%s: a batch needs n %% 4 == 0 (every image's row starts 16-byte aligned)", name);
  hipLaunchKernelGGL(randn_kernel, dim3(grid_for((long long)B * ((n + 3) / 4))), dim3(256), 0, (hipStream_t)stream, out, B, n,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), step_dev, step_const, (unsigned)sub, img0, img_stride);
  return osm::check_launch("randn_kernel");
}
}  // namespace

extern "C" int osm_posterior_typed(const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind,
                                   int clip_denoised, float* x0_raw, float* x0, float* mean, float* logvar, int B, int HW,
                                   void* stream) {
  OSM_REQUIRE(model_out && x && coef && x0 && mean && logvar && B > 0 && HW > 0, "osm_posterior_typed: bad argument");
  OSM_REQUIRE(!clip_denoised || x0_raw, "osm_posterior_typed: clip_denoised needs x0_raw (the unclamped prediction, read by osm_clamp_bwd)");
  int rc = check_kinds("osm_posterior_typed", mean_kind, var_kind);
  if (rc) return rc;
  return posterior_launch(false, model_out, x, coef, mean_kind, var_kind, clip_denoised ? x0_raw : nullptr, x0, mean, logvar, B, 4, 8,
                          HW, (hipStream_t)stream);
}

extern "C" int osm_posterior_c(const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind,
                               int clip_denoised, float* x0_raw, float* x0, float* mean, float* logvar, int B, int C, int Cout,
                               int HW, void* stream) {
  OSM_REQUIRE(model_out && x && coef && x0 && mean && logvar && B > 0 && HW > 0, "osm_posterior_c: bad argument");
  OSM_REQUIRE(!clip_denoised || x0_raw, "osm_posterior_c: clip_denoised needs x0_raw (the unclamped prediction, read by osm_clamp_bwd)");
  int rc = check_kinds("osm_posterior_c", mean_kind, var_kind);
  if (rc || (rc = check_cout("osm_posterior_c", C, Cout))) return rc;
  return posterior_launch(false, model_out, x, coef, mean_kind, var_kind, clip_denoised ? x0_raw : nullptr, x0, mean, logvar, B, C,
                          Cout, HW, (hipStream_t)stream);
}

extern "C" int osm_posterior(const float* model_out, const float* x, const float* coef, float* x0, float* mean,
                             float* logvar, int B, int HW, void* stream) {
  return osm_posterior_typed(model_out, x, coef, 0, 0, 0, nullptr, x0, mean, logvar, B, HW, stream);
}

extern "C" int osm_posterior_dynthr(const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind, float s,
                                    float* x0_raw, float* x0, float* mean, float* logvar, float* q, int* idx, void* ws, int B, int HW,
                                    void* stream) {
  OSM_REQUIRE(model_out && x && coef && x0_raw && x0 && mean && logvar && q && idx && ws && B > 0 && HW > 0,
              "osm_posterior_dynthr: bad argument");
  int rc = check_kinds("osm_posterior_dynthr", mean_kind, var_kind);
  if (rc) return rc;
  const long long total = (long long)B * 4 * HW;
  OSM_REQUIRE(total <= (1LL << 24), "osm_posterior_dynthr: quantile() input tensor is too large (%lld elements > 2^24)", total);
  return posterior_dynthr_launch(model_out, x, coef, mean_kind, var_kind, s, x0_raw, x0, mean, logvar, q, idx, ws, B, 4, 8, HW, stream);
}

extern "C" int osm_posterior_dynthr_c(const float* model_out, const float* x, const float* coef, int mean_kind, int var_kind, float s,
                                      float* x0_raw, float* x0, float* mean, float* logvar, float* q, int* idx, void* ws, int B, int C,
                                      int Cout, int HW, void* stream) {
  OSM_REQUIRE(model_out && x && coef && x0_raw && x0 && mean && logvar && q && idx && ws && B > 0 && C > 0 && HW > 0,
              "osm_posterior_dynthr_c: bad argument");
  const long long total = (long long)B * C * HW;
  OSM_REQUIRE(total <= (1LL << 24), "osm_posterior_dynthr_c: quantile() input tensor is too large (%lld elements > 2^24)", total);
  int rc = check_kinds("osm_posterior_dynthr_c", mean_kind, var_kind);
  if (rc || (rc = check_cout("osm_posterior_dynthr_c", C, Cout))) return rc;
  return posterior_dynthr_launch(model_out, x, coef, mean_kind, var_kind, s, x0_raw, x0, mean, logvar, q, idx, ws, B, C, Cout, HW,
                                 stream);
}

extern "C" int osm_clamp_bwd(float* g, const float* x_raw, float lo, float hi, long long n, void* stream) {
  OSM_REQUIRE(g && x_raw && n > 0 && lo <= hi, "osm_clamp_bwd: bad argument");
  hipLaunchKernelGGL(clamp_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, g, x_raw, lo, hi, n);
  return osm::check_launch("clamp_bwd_kernel");
}

extern "C" int osm_posterior_bwd(const float* g, const float* coef, float* d_out, int B, int HW, void* stream) {
  return posterior_bwd_launch("osm_posterior_bwd", g, coef, d_out, B, 4, 8, HW, stream);
}

extern "C" int osm_posterior_bwd_c(const float* g, const float* coef, float* d_out, int B, int C, int Cout, int HW, void* stream) {
  return posterior_bwd_launch("osm_posterior_bwd_c", g, coef, d_out, B, C, Cout, HW, stream);
}

extern "C" int osm_guide_update(const float* mean, const float* logvar, const float* g, const float* dx_unet,
                                const float* noise, const float* coef, const float* scale4, float clip,
                                float* x_next, float* grad_out, int B, int HW, void* stream) {
  return guide_update_launch("osm_guide_update", mean, logvar, g, dx_unet, noise, coef, scale4, clip, x_next, grad_out, B, 4, HW, stream);
}

extern "C" int osm_guide_update_c(const float* mean, const float* logvar, const float* g, const float* dx_unet, const float* noise,
                                  const float* coef, const float* scale, float clip, float* x_next, float* grad_out, int B, int C,
                                  int HW, void* stream) {
  return guide_update_launch("osm_guide_update_c", mean, logvar, g, dx_unet, noise, coef, scale, clip, x_next, grad_out, B, C, HW, stream);
}

extern "C" int osm_guide_update_rng(const float* mean, const float* logvar, const float* g, const float* dx_unet,
                                    const float* coef, const float* scale4, float clip, float* x_next, float* grad_out,
                                    float* noise_out, int B, int HW, unsigned long long seed, const int* step, int step_offset,
                                    int img0, int img_stride, void* stream) {
  return guide_update_rng_launch("osm_guide_update_rng", mean, logvar, g, dx_unet, coef, scale4, clip, x_next, grad_out, noise_out,
                                 B, 4, HW, seed, step, step_offset, 0, img0, img_stride, stream);
}

extern "C" int osm_guide_update_rng_sub(const float* mean, const float* logvar, const float* g, const float* dx_unet,
                                        const float* coef, const float* scale4, float clip, float* x_next, float* grad_out,
                                        float* noise_out, int B, int HW, unsigned long long seed, const int* step, int step_offset,
                                        int sub, int img0, int img_stride, void* stream) {
  return guide_update_rng_launch("osm_guide_update_rng_sub", mean, logvar, g, dx_unet, coef, scale4, clip, x_next, grad_out,
                                 noise_out, B, 4, HW, seed, step, step_offset, sub, img0, img_stride, stream);
}

extern "C" int osm_guide_update_rng_c(const float* mean, const float* logvar, const float* g, const float* dx_unet, const float* coef,
                                      const float* scale, float clip, float* x_next, float* grad_out, float* noise_out, int B, int C,
                                      int HW, unsigned long long seed, const int* step, int step_offset, int sub, int img0,
                                      int img_stride, void* stream) {
  return guide_update_rng_launch("osm_guide_update_rng_c", mean, logvar, g, dx_unet, coef, scale, clip, x_next, grad_out, noise_out, B,
                                 C, HW, seed, step, step_offset, sub, img0, img_stride, stream);
}

extern "C" int osm_randn(float* out, int B, long long n, unsigned long long seed, const int* step_dev, int step_const, int img0,
                         int img_stride, void* stream) {
  return randn_launch("osm_randn", out, B, n, seed, step_dev, step_const, 0, img0, img_stride, stream);
}

extern "C" int osm_randn_sub(float* out, int B, long long n, unsigned long long seed, const int* step_dev, int step_const, int sub,
                             int img0, int img_stride, void* stream) {
  return randn_launch("osm_randn_sub", out, B, n, seed, step_dev, step_const, sub, img0, img_stride, stream);
}

extern "C" int osm_philox_raw(unsigned* out, long long n4, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                              void* stream) {
  OSM_REQUIRE(out && n4 > 0, "osm_philox_raw: bad argument");
  hipLaunchKernelGGL(philox_raw_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, out, n4, c1, c2, c3, k0, k1);
  return osm::check_launch("philox_raw_kernel");
}

extern "C" int osm_ddim_update(const float* x0, const float* x, const float* g, const float* dx_unet, const float* noise,
                               const float* coef, const float* dcoef, const float* scale4, float clip, float* x_next,
                               float* grad_out, int B, int HW, void* stream) {
  return ddim_update_launch("osm_ddim_update", x0, x, g, dx_unet, noise, coef, dcoef, scale4, clip, x_next, grad_out, B, 4, HW, stream);
}

extern "C" int osm_ddim_update_c(const float* x0, const float* x, const float* g, const float* dx_unet, const float* noise,
                                 const float* coef, const float* dcoef, const float* scale, float clip, float* x_next,
                                 float* grad_out, int B, int C, int HW, void* stream) {
  return ddim_update_launch("osm_ddim_update_c", x0, x, g, dx_unet, noise, coef, dcoef, scale, clip, x_next, grad_out, B, C, HW, stream);
}

extern "C" int osm_solver_update_c(const float* x0, const float* x, float* hist, const float* g, const float* dx_unet, const float* noise,
                                   const float* coef, const float* srow, const float* scale, float clip, float* x_next,
                                   float* grad_out, float* noise_out, int B, int C, int HW, void* stream) {
  const SolverArgs a{x0, x, hist, g, dx_unet, noise, coef, srow, scale, clip, x_next, grad_out, noise_out, B, C, HW};
  return solver_update_launch("osm_solver_update_c", a, stream);
}

extern "C" int osm_solver_update_rng_c(const float* x0, const float* x, float* hist, const float* g, const float* dx_unet,
                                       const float* coef, const float* srow, const float* scale, float clip, float* x_next,
                                       float* grad_out, float* noise_out, int B, int C, int HW, unsigned long long seed,
                                       const int* step, int step_offset, int sub, int img0, int img_stride, void* stream) {
  const SolverArgs a{x0, x, hist, g, dx_unet, nullptr, coef, srow, scale, clip, x_next, grad_out, noise_out, B, C, HW};
  return solver_update_rng_launch("osm_solver_update_rng_c", a, seed, step, step_offset, sub, img0, img_stride, stream);
}

extern "C" int osm_fetch_coefs(const float* table, int n_rows, int* step, int delta, float* coef_out, float* t_out,
                               int B, void* stream) {
  OSM_REQUIRE(table && step && coef_out && t_out && B > 0 && B <= 256 && n_rows > 0, "osm_fetch_coefs: bad argument");
  hipLaunchKernelGGL(fetch_coefs_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, table, step, delta, coef_out,
                     t_out, B, n_rows);
  return osm::check_launch("fetch_coefs_kernel");
}

extern "C" int osm_ancestral_step(const float* model_out, const float* x, const float* z, const float* coef,
                                  float* x_next, float* x0, int B, int C, int Cout, int HW, void* stream) {
  OSM_REQUIRE(model_out && x && coef && x_next && B > 0 && C > 0 && Cout >= C && HW > 0, "osm_ancestral_step: bad argument");
  hipLaunchKernelGGL(ancestral_step_kernel, dim3(grid_for((long long)B * C * HW)), dim3(256), 0, (hipStream_t)stream,
                     model_out, x, z, coef, x_next, x0, B, C, Cout, HW);
  return osm::check_launch("ancestral_step_kernel");
}

// ---------------------------------------------------------------- the 'ps' data term and the exposure mask
namespace {

// 'ps' data term on a C-channel x0 (condition_methods.py:35-41): per image, the partial sums of (y - x0[0:3])^2 in the order of
// phys_reduce_kernel (PPB pixels per workgroup, wave sums, the four waves pairwise): deterministic
// MASKED: the residual is M (y - x0[0:3]) with M [B,3,HW] laid out like y
template <bool MASKED>
__global__ __launch_bounds__(256) void ps_reduce_c_kernel(const float* __restrict__ x0, const float* __restrict__ y,
                                                           const float* __restrict__ mask, float* __restrict__ part, int C, int HW,
                                                           int nblk) {
  __shared__ float red[4];
  const int b = blockIdx.y, blk = blockIdx.x;
  const int pend = min(HW, (blk + 1) * PPB);
  const float* xb = x0 + (long long)b * C * HW;
  const float* yb = y + (long long)b * 3 * HW;
  float s = 0.f;
  for (int p = blk * PPB + threadIdx.x; p < pend; p += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float r = yb[(long long)c * HW + p] - xb[(long long)c * HW + p];
      if constexpr (MASKED) r *= mask[(long long)b * 3 * HW + (long long)c * HW + p];
      s += r * r;
    }
  }
  const float t = osm::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[(long long)b * nblk + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss[b] = sqrt(sum of the image's partials) (fp64, fixed order), g = -(y - x0) / loss on channels 0..2, 0 on any further channel
// MASKED: g = -M^2 (y - x0) / loss, and 0 for an image whose every pixel is masked out (loss = 0)
template <bool MASKED>
__global__ __launch_bounds__(256) void ps_grad_c_kernel(const float* __restrict__ x0, const float* __restrict__ y,
                                                         const float* __restrict__ mask,
                                                         const float* __restrict__ part, float* __restrict__ loss,
                                                         float* __restrict__ g, int C, int HW, int nblk) {
  __shared__ float tot;
  const int b = blockIdx.y;
  if (threadIdx.x < 64) {         // the first wave: lane l owns partials l, l + 64, ...; five shuffle folds
    double a = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) a += (double)part[(long long)b * nblk + k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
    if (threadIdx.x == 0) {
      tot = (float)a;
      if (blockIdx.x == 0) loss[b] = (float)sqrt(a);
    }
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  float gscale = 1.0f / sqrtf(tot);
  if constexpr (MASKED) {
    if (tot == 0.f) gscale = 0.f;
  }
  const long long base = (long long)b * C * HW + p;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r = y[(long long)b * 3 * HW + (long long)c * HW + p] - x0[base + (long long)c * HW];
    if constexpr (MASKED) {
      const float m = mask[(long long)b * 3 * HW + (long long)c * HW + p];
      g[base + (long long)c * HW] = -(m * ((m * r) * gscale));
    } else {
      g[base + (long long)c * HW] = -(r * gscale);
    }
  }
  for (int c = 3; c < C; ++c) g[base + (long long)c * HW] = 0.f;
}

// validity mask from the exposure of the measurement itself: y [B,3,HW] in [-1, 1], v = (y + 1) / 2 in [0, 1];
// soft > 0: M_c = clamp((hi - v) / soft, 0, 1) clamp((v - lo) / soft, 0, 1), a ramp of width `soft` inside each bound;
// soft = 0: M_c = [lo < v < hi].  per_pixel: every channel gets the minimum of the three (a clipped channel invalidates the pixel).
__global__ __launch_bounds__(256) void exposure_mask_kernel(const float* __restrict__ y, float lo, float hi, float soft, int per_pixel,
                                                             float* __restrict__ mask, int B, int HW) {
  const long long total = (long long)B * HW;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / HW, p = i - b * HW;
    const long long base = b * 3LL * HW + p;
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = 0.5f * (y[base + (long long)c * HW] + 1.0f);
      if (soft > 0.f) {
        const float a = fminf(fmaxf((hi - v) / soft, 0.f), 1.f), bl = fminf(fmaxf((v - lo) / soft, 0.f), 1.f);
        m[c] = a * bl;
      } else {
        m[c] = (v > lo && v < hi) ? 1.f : 0.f;
      }
    }
    if (per_pixel) m[0] = m[1] = m[2] = fminf(m[0], fminf(m[1], m[2]));
#pragma unroll
    for (int c = 0; c < 3; ++c) mask[base + (long long)c * HW] = m[c];
  }
}
}  // namespace

namespace {
int ps_loss_grad_launch(const char* who, const float* x0, const float* y, const float* mask, float* part, float* loss, float* g, int B,
                        int C, int HW, void* stream) {
  OSM_REQUIRE(x0 && y && part && loss && g && B > 0 && HW > 0, "%s: bad argument", who);
  OSM_REQUIRE(C >= 3, "%s: the data term reads channels 0..2 of x0, got C = %d", who, C);
  const int nblk = osm_phys_nblk(HW);
  const dim3 rgrid(nblk, B), ggrid((HW + 255) / 256, B);
  hipStream_t st = (hipStream_t)stream;
  if (mask) hipLaunchKernelGGL(ps_reduce_c_kernel<true>, rgrid, dim3(256), 0, st, x0, y, mask, part, C, HW, nblk);
  else hipLaunchKernelGGL(ps_reduce_c_kernel<false>, rgrid, dim3(256), 0, st, x0, y, nullptr, part, C, HW, nblk);
  int rc = osm::check_launch("ps_reduce_c_kernel");
  if (rc) return rc;
  if (mask) hipLaunchKernelGGL(ps_grad_c_kernel<true>, ggrid, dim3(256), 0, st, x0, y, mask, part, loss, g, C, HW, nblk);
  else hipLaunchKernelGGL(ps_grad_c_kernel<false>, ggrid, dim3(256), 0, st, x0, y, nullptr, part, loss, g, C, HW, nblk);
  return osm::check_launch("ps_grad_c_kernel");
}
}  // namespace

extern "C" int osm_ps_loss_grad_c(const float* x0, const float* y, float* part, float* loss, float* g, int B, int C, int HW,
                                  void* stream) {
  return ps_loss_grad_launch("osm_ps_loss_grad_c", x0, y, nullptr, part, loss, g, B, C, HW, stream);
}

extern "C" int osm_ps_loss_grad_mc(const float* x0, const float* y, const float* mask, float* part, float* loss, float* g, int B, int C,
                                   int HW, void* stream) {
  return ps_loss_grad_launch("osm_ps_loss_grad_mc", x0, y, mask, part, loss, g, B, C, HW, stream);
}

extern "C" int osm_exposure_mask(const float* y, float lo, float hi, float soft, int per_pixel, float* mask_out, int B, int HW,
                                 void* stream) {
  OSM_REQUIRE(y && mask_out && B > 0 && HW > 0, "osm_exposure_mask: bad argument");
  OSM_REQUIRE(lo <= hi, "osm_exposure_mask: low must not exceed high, got %g > %g", (double)lo, (double)hi);
  OSM_REQUIRE(soft >= 0.f, "osm_exposure_mask: soft must be >= 0, got %g", (double)soft);
  hipLaunchKernelGGL(exposure_mask_kernel, dim3(grid_for((long long)B * HW)), dim3(256), 0, (hipStream_t)stream, y, lo, hi, soft,
                     per_pixel, mask_out, B, HW);
  return osm::check_launch("exposure_mask_kernel");
}
