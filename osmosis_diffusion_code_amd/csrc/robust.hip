// A robust data term (include/osmosis_robust.h, which is the contract: the reference has no such term).  Per guided sub-step and per
// image: the raw residual e = y - (pa pred + pb) on the measurement's grid, a robust scale sigma = 1.4826 median |e| over the valid
// entries, and per-entry IRLS weights omega(|e| / (c sigma)) folded into the mask the existing masked data term reads.
//   robust_resid_kernel   grid (ceil(3 hw / 256), B): e, three fp32 operations of one rounding each, never an fma
//   robust_scale_kernel   ONE 1024-lane workgroup per image: exact radix select (digits 11 / 10 / 10 of the 31-bit keys of |e|, the
//                         split of select.hip) over the entries with M0 > 0 and e finite, both median ranks followed at once;
//                         histograms in LDS with integer atomics (exact: the counts do not depend on the schedule); n_b from pass 0
//   robust_weight_kernel  grid (ceil(hw / 256), B), one lane per pixel and its three channels (per_pixel needs them together)
// No global atomics, nothing shared between workgroups: bit-reproducible, and the bits of an image do not depend on the batch.
// Latency-bound: the select reads e and M0 three times (3 x 1.5 MB at 256 x 256) from one CU per image.
#include "osm_common.h"
#include "../../include/osmosis_robust.h"

namespace {

constexpr int RS_T = 1024;       // lanes of the select workgroup
constexpr int RS_BIN = 2048;     // pass 0: 2048 digits; passes 1-2: 2 targets x 1024
constexpr unsigned KEY_INF = 0x7f800000u;

__global__ __launch_bounds__(256) void robust_resid_kernel(const float* __restrict__ pred, const long long bstride, const float pa,
                                                           const float pb, const float* __restrict__ y, float* __restrict__ e,
                                                           const int n) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float t = __fmul_rn(pa, pred[(long long)b * bstride + i]);
  const float P = __fadd_rn(t, pb);
  e[(long long)b * n + i] = __fsub_rn(y[(long long)b * n + i], P);
}

// exclusive prefix sum of v over the RS_T-lane workgroup; every lane must call it
__device__ unsigned block_excl_scan(unsigned v, unsigned* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) red[wid] = inc;
  __syncthreads();
  unsigned base = 0;
  for (int w = 0; w < wid; ++w) base += red[w];
  __syncthreads();
  return base + inc - v;
}

// the key of entry i when it is valid (M0 > 0 and e finite)
__device__ __forceinline__ bool valid_key(const float* __restrict__ eb, const float* __restrict__ mb, int i, unsigned& k) {
  k = __float_as_uint(eb[i]) & 0x7fffffffu;
  if (k >= KEY_INF) return false;
  return mb == nullptr || mb[i] > 0.0f;
}

__global__ __launch_bounds__(RS_T) void robust_scale_kernel(const float* __restrict__ e, const float* __restrict__ m0,
                                                            float* __restrict__ sigma, int* __restrict__ n_valid, const int n,
                                                            const float sigma_min) {
  __shared__ unsigned h[RS_BIN];
  __shared__ unsigned red[RS_T / 64];
  __shared__ unsigned pre_s[2], rank_s[2], n_s;
  const int b = blockIdx.x, t = threadIdx.x;
  const float* __restrict__ eb = e + (long long)b * n;
  const float* __restrict__ mb = m0 ? m0 + (long long)b * n : nullptr;

  // pass 0: the top 11 bits of every valid key; the histogram's total is n_b
  for (int i = t; i < RS_BIN; i += RS_T) h[i] = 0u;
  __syncthreads();
  for (int i = t; i < n; i += RS_T) {
    unsigned k;
    if (valid_key(eb, mb, i, k)) atomicAdd(&h[k >> 20], 1u);
  }
  __syncthreads();
  {
    const unsigned a = h[2 * t], c = h[2 * t + 1];
    const unsigned ex = block_excl_scan(a + c, red);
    if (t == RS_T - 1) n_s = ex + a + c;
    __syncthreads();
    const unsigned nb = n_s;
    if (nb == 0u) {                       // (uniform: every lane reads the same n_s)
      if (t == 0) {
        sigma[b] = __uint_as_float(0x7fc00000u);
        n_valid[b] = 0;
      }
      return;
    }
    const unsigned rk[2] = {(nb - 1u) >> 1, nb >> 1};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (rk[q] >= ex && rk[q] < ex + a) {
        pre_s[q] = (unsigned)(2 * t) << 20;
        rank_s[q] = rk[q] - ex;
      } else if (rk[q] >= ex + a && rk[q] < ex + a + c) {
        pre_s[q] = (unsigned)(2 * t + 1) << 20;
        rank_s[q] = rk[q] - ex - a;
      }
    }
    __syncthreads();
  }

  // passes 1 and 2: the next 10 bits of the keys that carry each target's prefix
#pragma unroll 1
  for (int pass = 1; pass < 3; ++pass) {
    const int shift = pass == 1 ? 10 : 0;
    const unsigned fixed = pass == 1 ? 0x7ff00000u : 0x7ffffc00u;
    const unsigned pre[2] = {pre_s[0], pre_s[1]}, rk[2] = {rank_s[0], rank_s[1]};
    const bool same = pre[0] == pre[1];
    for (int i = t; i < RS_BIN; i += RS_T) h[i] = 0u;
    __syncthreads();                      // (also: every lane has read pre_s / rank_s before anyone rewrites them)
    for (int i = t; i < n; i += RS_T) {
      unsigned k;
      if (!valid_key(eb, mb, i, k)) continue;
      const unsigned dg = (k >> shift) & 1023u;
      if ((k & fixed) == pre[0]) atomicAdd(&h[dg], 1u);
      if (!same && (k & fixed) == pre[1]) atomicAdd(&h[1024 + dg], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const unsigned c = h[(same ? 0 : q * 1024) + t];
      const unsigned ex = block_excl_scan(c, red);
      if (rk[q] >= ex && rk[q] < ex + c) {
        pre_s[q] = pre[q] | ((unsigned)t << shift);
        rank_s[q] = rk[q] - ex;
      }
    }
    __syncthreads();
  }

  if (t == 0) {
    const float a_lo = __uint_as_float(pre_s[0]), a_hi = __uint_as_float(pre_s[1]);
    const float med = __fmul_rn(0.5f, __fadd_rn(a_lo, a_hi));
    sigma[b] = fmaxf(__fmul_rn(1.4826f, med), sigma_min);
    n_valid[b] = (int)n_s;
  }
}

__global__ __launch_bounds__(256) void robust_weight_kernel(const osm_robust_desc ds, const float* __restrict__ e,
                                                            const float* __restrict__ m0, const float* __restrict__ sigma,
                                                            float* __restrict__ meff, float* __restrict__ omega) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ds.hw) return;
  const float sg = ds.scale_mode == 1 ? ds.scale : sigma[b];
  const float cs = __fmul_rn(ds.c, sg);
  const long long base = (long long)b * 3 * ds.hw + p;
  float mv[3], u[3];
  bool ok[3];
  float umax = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long i = base + (long long)c * ds.hw;
    const float ev = e[i];
    mv[c] = m0 ? m0[i] : 1.0f;
    const float ae = fabsf(ev);
    ok[c] = (__float_as_uint(ae) < KEY_INF) && mv[c] > 0.0f && sg == sg;     // sg NaN: n_b = 0, nothing is valid
    u[c] = ae == 0.0f ? 0.0f : __fdiv_rn(ae, cs);
    if (ok[c]) umax = fmaxf(umax, u[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long i = base + (long long)c * ds.hw;
    float w = 1.0f, out = mv[c];
    if (ok[c]) {
      const float uu = ds.per_pixel ? umax : u[c];
      float s;                             // sqrt(omega)
      if (ds.loss == 0) {
        w = uu <= 1.0f ? 1.0f : __fdiv_rn(1.0f, uu);
        s = __fsqrt_rn(w);
      } else if (ds.loss == 1) {
        s = uu < 1.0f ? __fsub_rn(1.0f, __fmul_rn(uu, uu)) : 0.0f;
        w = __fmul_rn(s, s);
      } else {
        w = __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(uu, uu)));
        s = __fsqrt_rn(w);
      }
      out = __fmul_rn(mv[c], s);
    }
    meff[i] = out;
    if (omega) omega[i] = w;
  }
}

int check_desc(const char* what, const osm_robust_desc* d) {
  OSM_REQUIRE(d, "%s: null pointer (the descriptor)", what);
  OSM_REQUIRE(d->loss >= 0 && d->loss <= 2, "%s: unknown loss %d (0 huber, 1 tukey, 2 cauchy)", what, d->loss);
  OSM_REQUIRE(d->c > 0.0f && d->c <= 3.0e38f, "%s: c must be finite and > 0, got %g", what, (double)d->c);
  OSM_REQUIRE(d->scale_mode == 0 || d->scale_mode == 1, "%s: unknown scale_mode %d (0 mad, 1 fixed)", what, d->scale_mode);
  OSM_REQUIRE(d->scale_mode == 0 || (d->scale > 0.0f && d->scale <= 3.0e38f), "%s: a fixed scale must be finite and > 0, got %g", what,
              (double)d->scale);
  OSM_REQUIRE(d->sigma_min >= 0.0f && d->sigma_min <= 3.0e38f, "%s: sigma_min must be finite and >= 0, got %g", what,
              (double)d->sigma_min);
  OSM_REQUIRE(d->per_pixel == 0 || d->per_pixel == 1, "%s: per_pixel must be 0 or 1, got %d", what, d->per_pixel);
  OSM_REQUIRE(d->B > 0 && d->hw > 0, "%s: bad shape B %d, hw %d", what, d->B, d->hw);
  OSM_REQUIRE(d->B <= 65535 && d->hw < (1 << 29), "%s: B %d / hw %d are too many for one launch", what, d->B, d->hw);
  return OSM_OK;
}

int check_pred(const char* what, const osm_robust_desc* d, long long bstride, float pa, float pb) {
  OSM_REQUIRE(bstride >= 3LL * d->hw, "%s: pred_bstride %lld is smaller than the three planes 3 hw = %lld", what, bstride, 3LL * d->hw);
  OSM_REQUIRE(pa >= -3.0e38f && pa <= 3.0e38f && pb >= -3.0e38f && pb <= 3.0e38f, "%s: pa / pb must be finite, got %g and %g", what,
              (double)pa, (double)pb);
  return OSM_OK;
}

void launch_resid(const osm_robust_desc* d, const float* pred, long long bstride, float pa, float pb, const float* y, float* e,
                  hipStream_t st) {
  const int n = 3 * d->hw;
  hipLaunchKernelGGL(robust_resid_kernel, dim3((n + 255) / 256, d->B), dim3(256), 0, st, pred, bstride, pa, pb, y, e, n);
}

void launch_scale(const osm_robust_desc* d, const float* e, const float* M0, float* sigma, int* n_valid, hipStream_t st) {
  hipLaunchKernelGGL(robust_scale_kernel, dim3(d->B), dim3(RS_T), 0, st, e, M0, sigma, n_valid, 3 * d->hw, d->sigma_min);
}

void launch_weights(const osm_robust_desc* d, const float* e, const float* M0, const float* sigma, float* M_eff, float* omega,
                    hipStream_t st) {
  hipLaunchKernelGGL(robust_weight_kernel, dim3((d->hw + 255) / 256, d->B), dim3(256), 0, st, *d, e, M0, sigma, M_eff, omega);
}

}  // namespace

extern "C" int osm_robust_resid(const osm_robust_desc* d, const float* pred, long long pred_bstride, float pa, float pb, const float* y,
                                float* e, void* stream) {
  const char* what = "osm_robust_resid";
  int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(pred && y && e, "%s: null pointer (pred / y / e)", what);
  rc = check_pred(what, d, pred_bstride, pa, pb);
  if (rc) return rc;
  launch_resid(d, pred, pred_bstride, pa, pb, y, e, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_robust_scale(const osm_robust_desc* d, const float* e, const float* M0, float* sigma, int* n_valid, void* stream) {
  const char* what = "osm_robust_scale";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(e && sigma && n_valid, "%s: null pointer (e / sigma / n_valid)", what);
  launch_scale(d, e, M0, sigma, n_valid, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_robust_weights(const osm_robust_desc* d, const float* e, const float* M0, const float* sigma, float* M_eff,
                                  float* omega, void* stream) {
  const char* what = "osm_robust_weights";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(e && M_eff, "%s: null pointer (e / M_eff)", what);
  OSM_REQUIRE(sigma || d->scale_mode == 1, "%s: null pointer (sigma, which the mad scale reads)", what);
  launch_weights(d, e, M0, sigma, M_eff, omega, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_robust_mask(const osm_robust_desc* d, const float* pred, long long pred_bstride, float pa, float pb, const float* y,
                               const float* M0, float* e, float* sigma, int* n_valid, float* M_eff, float* omega, void* stream) {
  const char* what = "osm_robust_mask";
  int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(pred && y && e && M_eff, "%s: null pointer (pred / y / e / M_eff)", what);
  OSM_REQUIRE(d->scale_mode == 1 || (sigma && n_valid), "%s: null pointer (sigma / n_valid, which the mad scale writes)", what);
  rc = check_pred(what, d, pred_bstride, pa, pb);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_resid(d, pred, pred_bstride, pa, pb, y, e, st);
  if (d->scale_mode == 0) launch_scale(d, e, M0, sigma, n_valid, st);
  launch_weights(d, e, M0, sigma, M_eff, omega, st);
  return osm::check_launch(what);
}
