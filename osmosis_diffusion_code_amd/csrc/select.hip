// Exact order statistics of |x| on the device, and the backward of dynamic thresholding through them.
//   quantile of |x| with linear interpolation        util/img_utils.py:8-15 (torch.quantile(img.abs(), s))
//   d/dx of clip(x * quantile(|x|, s), -1, 1)           autograd of the same line (posterior_mean_variance.py:43-50)
//
// Select: radix select on the 31-bit keys bits(x) & 0x7fffffff (monotone in |x|; +-0 share a key; +inf < NaN), three digit
// passes of 11 / 10 / 10 bits for the two order statistics of the interpolation at once, then the stable index of each (the
// (k - #smaller)-th occurrence of the key in index order).  Workgroups share work only through stream order: per-workgroup
// LDS histograms flushed with integer atomics (exact, so the counts do not depend on the schedule), and single-workgroup scan
// kernels that read them in the next launch.  Every streaming workgroup owns SEL_CHUNK contiguous elements.
#include "osm_common.h"

namespace {

constexpr int SEL_T = 256;                    // threads of a streaming workgroup
constexpr int SEL_EPT = 8;                    // elements per thread of a streaming workgroup
constexpr int SEL_CHUNK = SEL_T * SEL_EPT;    // contiguous elements per streaming workgroup
constexpr int SCAN_T = 1024;                  // threads of the single-workgroup kernels
constexpr int NBIN = 2048;                    // histogram bins of a pass (pass 0: 2048 digits; passes 1-2: 2 targets x 1024)
constexpr long long SEL_MAX_N = 1LL << 24;    // torch.quantile's own limit
constexpr int SEL_MAX_BLK = (int)(SEL_MAX_N / SEL_CHUNK);
constexpr int CNT_PT = SEL_MAX_BLK / SCAN_T;  // per-workgroup counts per thread of the find kernel
constexpr int CHUNK_PT = SEL_CHUNK / SCAN_T;  // elements per thread when the find kernel walks one chunk
constexpr unsigned NAN_KEY0 = 0x7f800001u;    // keys above +inf are NaN
constexpr int ST_WORDS = 8;

// workspace (32-bit words): state[8] | hist[3][NBIN] | cnt[2][nblk]
//   state: 0-1 key prefix of target 0 (rank lo) / 1 (rank hi), 2-3 rank among the elements with that prefix, 4 NaN count,
//          5 prefixes equal (the two targets share a histogram)
enum { S_PRE = 0, S_RANK = 2, S_NAN = 4, S_SAME = 5 };

__device__ __forceinline__ unsigned key_of(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exclusive prefix sum of v over a SCAN_T-thread workgroup; every thread must call it
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

__global__ __launch_bounds__(SCAN_T) void sel_init_kernel(unsigned* __restrict__ ws, unsigned lo, unsigned hi) {
  for (int i = threadIdx.x; i < ST_WORDS + 3 * NBIN; i += SCAN_T) ws[i] = 0u;
  if (threadIdx.x == 0) {
    ws[S_RANK] = lo;
    ws[S_RANK + 1] = hi;
    ws[S_SAME] = 1u;
  }
}

// histogram of digit PASS of the keys that carry the prefix of each target (pass 0: of every key, plus the NaN count)
template <int PASS>
__global__ __launch_bounds__(SEL_T) void sel_hist_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ ws) {
  constexpr int SHIFT = PASS == 0 ? 20 : (PASS == 1 ? 10 : 0);
  constexpr unsigned FIXED = PASS == 0 ? 0u : (PASS == 1 ? 0x7ff00000u : 0x7ffffc00u);
  __shared__ unsigned h[NBIN];
  for (int i = threadIdx.x; i < NBIN; i += SEL_T) h[i] = 0u;
  const unsigned p0 = ws[S_PRE], p1 = ws[S_PRE + 1];
  const bool same = ws[S_SAME] != 0u;
  __syncthreads();
  const long long base = (long long)blockIdx.x * SEL_CHUNK + threadIdx.x;
  unsigned nan = 0;
#pragma unroll
  for (int j = 0; j < SEL_EPT; ++j) {
    const long long i = base + (long long)j * SEL_T;
    if (i < n) {
      const unsigned k = key_of(x[i]);
      if (PASS == 0) {
        atomicAdd(&h[k >> SHIFT], 1u);
        nan += k >= NAN_KEY0 ? 1u : 0u;
      } else {
        const unsigned d = (k >> SHIFT) & 1023u;
        if ((k & FIXED) == p0) atomicAdd(&h[d], 1u);
        if (!same && (k & FIXED) == p1) atomicAdd(&h[1024 + d], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* hist = ws + ST_WORDS + PASS * NBIN;
  for (int i = threadIdx.x; i < NBIN; i += SEL_T)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  if (PASS == 0) {
    nan = wave_sum_u(nan);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&ws[S_NAN], nan);
  }
}

// one workgroup: the digit of each target's order statistic (the bucket whose cumulative count straddles its rank)
template <int PASS>
__global__ __launch_bounds__(SCAN_T) void sel_scan_kernel(unsigned* __restrict__ ws) {
  constexpr int SHIFT = PASS == 0 ? 20 : (PASS == 1 ? 10 : 0);
  __shared__ unsigned red[SCAN_T / 64];
  __shared__ unsigned pre_s[2], rank_s[2];
  const unsigned* hist = ws + ST_WORDS + PASS * NBIN;
  const unsigned rank[2] = {ws[S_RANK], ws[S_RANK + 1]};
  const unsigned pre[2] = {ws[S_PRE], ws[S_PRE + 1]};
  const bool same = ws[S_SAME] != 0u;
  const unsigned t = threadIdx.x;
  if (PASS == 0) {
    const unsigned a = hist[2 * t], b = hist[2 * t + 1];
    const unsigned ex = block_excl_scan(a + b, red);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const unsigned k = rank[q];
      if (k >= ex && k < ex + a) {
        pre_s[q] = (2 * t) << SHIFT;
        rank_s[q] = k - ex;
      } else if (k >= ex + a && k < ex + a + b) {
        pre_s[q] = (2 * t + 1) << SHIFT;
        rank_s[q] = k - ex - a;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const unsigned c = hist[(same ? 0 : q * 1024) + t];
      const unsigned ex = block_excl_scan(c, red);
      const unsigned k = rank[q];
      if (k >= ex && k < ex + c) {
        pre_s[q] = pre[q] | (t << SHIFT);
        rank_s[q] = k - ex;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    ws[S_PRE] = pre_s[0];
    ws[S_PRE + 1] = pre_s[1];
    ws[S_RANK] = rank_s[0];
    ws[S_RANK + 1] = rank_s[1];
    ws[S_SAME] = pre_s[0] == pre_s[1] ? 1u : 0u;
  }
}

// per-workgroup occurrences of the two selected keys (in chunk order)
__global__ __launch_bounds__(SEL_T) void sel_count_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ ws,
                                                          int nblk) {
  __shared__ unsigned red[2][SEL_T / 64];
  const unsigned k0 = ws[S_PRE], k1 = ws[S_PRE + 1];
  const long long base = (long long)blockIdx.x * SEL_CHUNK + threadIdx.x;
  unsigned c0 = 0, c1 = 0;
#pragma unroll
  for (int j = 0; j < SEL_EPT; ++j) {
    const long long i = base + (long long)j * SEL_T;
    if (i < n) {
      const unsigned k = key_of(x[i]);
      c0 += k == k0 ? 1u : 0u;
      c1 += k == k1 ? 1u : 0u;
    }
  }
  c0 = wave_sum_u(c0);
  c1 = wave_sum_u(c1);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = c0;
    red[1][threadIdx.x >> 6] = c1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned s0 = 0, s1 = 0;
    for (int w = 0; w < SEL_T / 64; ++w) {
      s0 += red[0][w];
      s1 += red[1][w];
    }
    unsigned* cnt = ws + ST_WORDS + 3 * NBIN;
    cnt[blockIdx.x] = s0;
    cnt[nblk + blockIdx.x] = s1;
  }
}

// one workgroup: the stable index of each order statistic (which chunk holds its occurrence, then where in the chunk), and q
__global__ __launch_bounds__(SCAN_T) void sel_find_kernel(const float* __restrict__ x, long long n, const unsigned* __restrict__ ws,
                                                         int nblk, float w, float* __restrict__ q_out, int* __restrict__ idx_out) {
  __shared__ unsigned red[SCAN_T / 64];
  __shared__ unsigned blk_s, r_s;
  __shared__ int found[2];
  const unsigned* cnt = ws + ST_WORDS + 3 * NBIN;
  const int t = threadIdx.x;
  if (t < 2) found[t] = 0;
  if (t == 0) blk_s = r_s = 0u;
#pragma unroll 1
  for (int q = 0; q < 2; ++q) {
    const unsigned key = ws[S_PRE + q], r = ws[S_RANK + q];
    unsigned c[CNT_PT], s = 0;
#pragma unroll
    for (int e = 0; e < CNT_PT; ++e) {
      const int b = t * CNT_PT + e;
      c[e] = b < nblk ? cnt[q * nblk + b] : 0u;
      s += c[e];
    }
    unsigned ex = block_excl_scan(s, red);
    if (r >= ex && r < ex + s) {
#pragma unroll
      for (int e = 0; e < CNT_PT; ++e) {
        if (r >= ex && r < ex + c[e]) {
          blk_s = (unsigned)(t * CNT_PT + e);
          r_s = r - ex;
        }
        ex += c[e];
      }
    }
    __syncthreads();
    const long long base = (long long)blk_s * SEL_CHUNK + (long long)t * CHUNK_PT;
    const unsigned rr = r_s;
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < CHUNK_PT; ++e) m += (base + e < n && key_of(x[base + e]) == key) ? 1u : 0u;
    ex = block_excl_scan(m, red);
    if (rr >= ex && rr < ex + m) {
      unsigned seen = ex;
#pragma unroll
      for (int e = 0; e < CHUNK_PT; ++e) {
        if (base + e < n && key_of(x[base + e]) == key) {
          if (seen == rr) found[q] = (int)(base + e);
          ++seen;
        }
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    idx_out[0] = found[0];
    idx_out[1] = found[1];
    const float v0 = __uint_as_float(ws[S_PRE]), v1 = __uint_as_float(ws[S_PRE + 1]);
    const float d = v1 - v0;
    // torch.lerp's two-branch form; any NaN in the input makes the quantile NaN (ATen moves the rank onto the sorted NaN)
    const float qv = fabsf(w) < 0.5f ? v0 + w * d : v1 - d * (1.0f - w);
    q_out[0] = ws[S_NAN] ? __uint_as_float(0x7fc00000u) : qv;
  }
}

__device__ __forceinline__ float sgn_f(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }   // torch.sgn (NaN -> 0)

// g <- q m g in place (m = [-1 <= q x <= 1], ATen clamp_backward) and the workgroup's partial of S = sum m g x (fixed order)
__global__ __launch_bounds__(SEL_T) void dynthr_bwd_kernel(float* __restrict__ g, const float* __restrict__ x,
                                                           const float* __restrict__ q, long long n, float* __restrict__ part) {
  __shared__ float red[SEL_T / 64];
  const float qv = q[0];
  const long long base = (long long)blockIdx.x * SEL_CHUNK + threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < SEL_EPT; ++j) {
    const long long i = base + (long long)j * SEL_T;
    if (i < n) {
      const float xv = x[i], u = xv * qv;
      const float gm = (u >= -1.0f && u <= 1.0f) ? g[i] : 0.f;
      s += gm * xv;
      g[i] = qv * gm;
    }
  }
  s = osm::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < SEL_T / 64; ++w) t += red[w];
    part[blockIdx.x] = t;
  }
}

// one workgroup: S from the partials (fixed order), then the rank-one term of d quantile / dx at the two order statistics
__global__ __launch_bounds__(SCAN_T) void dynthr_rank1_kernel(float* __restrict__ g, const float* __restrict__ x,
                                                             const int* __restrict__ idx, const float* __restrict__ part, int nblk,
                                                             long long n, float w) {
  __shared__ float red[SCAN_T / 64];
  float s = 0.f;
  for (int b = threadIdx.x; b < nblk; b += SCAN_T) s += part[b];
  s = osm::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f;
    for (int i = 0; i < SCAN_T / 64; ++i) S += red[i];
    const int i0 = idx[0], i1 = idx[1];
    if (i0 >= 0 && i0 < n) g[i0] += sgn_f(x[i0]) * ((1.0f - w) * S);
    if (i1 >= 0 && i1 < n) g[i1] += sgn_f(x[i1]) * (w * S);
  }
}

inline int sel_blocks(long long n) { return (int)((n + SEL_CHUNK - 1) / SEL_CHUNK); }

// torch.quantile's rank, in the input's dtype: r = s (n - 1) in fp32, lo = floor(r), hi = ceil(r), w = r - lo
inline void sel_rank(float s, long long n, unsigned& lo, unsigned& hi, float& w) {
  const float r = s * (float)(n - 1);
  const float rf = floorf(r);
  lo = (unsigned)rf;
  hi = (unsigned)ceilf(r);
  w = r - rf;
}

}  // namespace

extern "C" long long osm_quantile_abs_ws_bytes(long long n) {
  if (n < 1 || n > SEL_MAX_N) return -1;
  return 4LL * (ST_WORDS + 3 * NBIN + 2LL * sel_blocks(n));
}

extern "C" int osm_quantile_abs(const float* x, long long n, float s, float* q, int* idx, void* ws, void* stream) {
  OSM_REQUIRE(x && q && idx && ws && n > 0, "osm_quantile_abs: bad argument");
  OSM_REQUIRE(n <= SEL_MAX_N, "osm_quantile_abs: quantile() input tensor is too large (%lld elements > 2^24)", n);
  OSM_REQUIRE(s >= 0.f && s <= 1.f, "osm_quantile_abs: q must be in the range [0, 1]");
  OSM_REQUIRE(osm::aligned16(ws), "osm_quantile_abs: workspace must be 16-byte aligned");
  unsigned lo, hi;
  float w;
  sel_rank(s, n, lo, hi, w);
  const int nblk = sel_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  unsigned* u = static_cast<unsigned*>(ws);
  hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(SCAN_T), 0, st, u, lo, hi);
  hipLaunchKernelGGL(sel_hist_kernel<0>, dim3(nblk), dim3(SEL_T), 0, st, x, n, u);
  hipLaunchKernelGGL(sel_scan_kernel<0>, dim3(1), dim3(SCAN_T), 0, st, u);
  hipLaunchKernelGGL(sel_hist_kernel<1>, dim3(nblk), dim3(SEL_T), 0, st, x, n, u);
  hipLaunchKernelGGL(sel_scan_kernel<1>, dim3(1), dim3(SCAN_T), 0, st, u);
  hipLaunchKernelGGL(sel_hist_kernel<2>, dim3(nblk), dim3(SEL_T), 0, st, x, n, u);
  hipLaunchKernelGGL(sel_scan_kernel<2>, dim3(1), dim3(SCAN_T), 0, st, u);
  hipLaunchKernelGGL(sel_count_kernel, dim3(nblk), dim3(SEL_T), 0, st, x, n, u, nblk);
  hipLaunchKernelGGL(sel_find_kernel, dim3(1), dim3(SCAN_T), 0, st, x, n, u, nblk, w, q, idx);
  return osm::check_launch("sel_find_kernel");
}

extern "C" int osm_dynthr_bwd(float* g, const float* x_raw, const float* q, const int* idx, float s, long long n, void* ws,
                              void* stream) {
  OSM_REQUIRE(g && x_raw && q && idx && ws && n > 0, "osm_dynthr_bwd: bad argument");
  OSM_REQUIRE(n <= SEL_MAX_N, "osm_dynthr_bwd: more than 2^24 elements");
  OSM_REQUIRE(s >= 0.f && s <= 1.f, "osm_dynthr_bwd: s must be in the range [0, 1]");
  unsigned lo, hi;
  float w;
  sel_rank(s, n, lo, hi, w);
  const int nblk = sel_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(dynthr_bwd_kernel, dim3(nblk), dim3(SEL_T), 0, st, g, x_raw, q, n, part);
  hipLaunchKernelGGL(dynthr_rank1_kernel, dim3(1), dim3(SCAN_T), 0, st, g, x_raw, idx, part, nblk, n, w);
  return osm::check_launch("dynthr_rank1_kernel");
}
