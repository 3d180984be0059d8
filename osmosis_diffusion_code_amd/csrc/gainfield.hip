// A learnt vignetting gain field in the Osmosis data term (include/osmosis_gain.h, which is the contract: the reference has no such
// term).  The photo is G F(x0; phi) with G the bilinear interpolation of a coarse node grid; the residual of that model is the existing
// masked residual on y' = (y + 1) / G - 1 with the mask M G, so per guided sub-step these kernels learn the nodes and write (y', M G):
//   gain_rows_kernel     grid (ceil(H / 4), B), one wave per pixel row: q = sum_c r_c dr_c/dG per pixel into an LDS row, then lane
//                        jx < gw sums hatx_jx(x) q over its node's support in ascending x; the row's sum of r^2 by a fixed xor tree
//   gain_step_kernel     one workgroup per image: c_raw and S in float64 over ascending y, the projected gradient step with the
//                        4-neighbour Laplacian and the gauge max n = 1, nodes in LDS
//   gain_expand_kernel   grid (ceil(H ceil(W / 4) / 256), B), a lane owns four consecutive pixels of a row (16-byte accesses when
//                        W % 4 == 0 and everything is aligned, scalar otherwise: the same bits), the image's nodes staged in LDS
// No atomics, nothing shared between workgroups: bit-reproducible, and the bits of an image do not depend on the batch.  All three are
// launch-bound at the sizes of a guided sub-step (1.3 MB of traffic at 256 x 256).
#include "osm_common.h"
#include "../../include/osmosis_gain.h"

// every product and every sum below is rounded once, in the order written (the Makefile passes -ffp-contract=off as well)
#pragma clang fp contract(off)

namespace {

constexpr int GAIN_MAX_G = 32;                    // nodes per side
constexpr int GAIN_MAX_W = 4096;                  // the LDS row buffers of gain_rows_kernel: 4 waves x W floats <= 64 KiB

struct GainTabs {
  const int* iy0;
  const float* fy;
  const int* ix0;
  const float* fx;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// G from the two node rows n0 (cell row iy0) and n1 (iy0 + 1), the column cell ix, fx, b = 1 - fy and fy
__device__ __forceinline__ float gain_at(const float* n0, const float* n1, int ix, float f, float bw, float fyv) {
  const float a = __fsub_rn(1.0f, f);
  const float top = __fadd_rn(__fmul_rn(a, n0[ix]), __fmul_rn(f, n0[ix + 1]));
  const float bot = __fadd_rn(__fmul_rn(a, n1[ix]), __fmul_rn(f, n1[ix + 1]));
  return __fadd_rn(__fmul_rn(bw, top), __fmul_rn(fyv, bot));
}

__device__ __forceinline__ void expand_px(float G, float y0, float y1, float y2, float m0, float m1, float m2, float& e0, float& e1,
                                          float& e2, float& o0, float& o1, float& o2) {
  e0 = __fsub_rn(__fdiv_rn(__fadd_rn(y0, 1.0f), G), 1.0f);
  e1 = __fsub_rn(__fdiv_rn(__fadd_rn(y1, 1.0f), G), 1.0f);
  e2 = __fsub_rn(__fdiv_rn(__fadd_rn(y2, 1.0f), G), 1.0f);
  o0 = __fmul_rn(m0, G);
  o1 = __fmul_rn(m1, G);
  o2 = __fmul_rn(m2, G);
}

__global__ __launch_bounds__(256) void gain_expand_kernel(const GainTabs tb, const float* __restrict__ nodes, const float* __restrict__ y,
                                                          const float* __restrict__ m0, float* __restrict__ ye, float* __restrict__ me,
                                                          float* __restrict__ field, const int H, const int W, const int gh,
                                                          const int gw, const int vec) {
  __shared__ float nl[GAIN_MAX_G * GAIN_MAX_G];
  const int b = blockIdx.y, ng = gh * gw;
  for (int i = threadIdx.x; i < ng; i += 256) nl[i] = nodes[(long long)b * ng + i];
  __syncthreads();
  const int qpr = (W + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= H * qpr) return;
  const int row = q / qpr, x0 = (q - row * qpr) * 4;
  const int iy = clampi(tb.iy0[row], gh - 2);
  const float fyv = tb.fy[row], bw = __fsub_rn(1.0f, fyv);
  const float* n0 = nl + iy * gw;
  const float* n1 = n0 + gw;
  const int nv = min(4, W - x0);
  float G[4] = {1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < nv) G[k] = gain_at(n0, n1, clampi(tb.ix0[x0 + k], gw - 2), tb.fx[x0 + k], bw, fyv);
  const long long HW = (long long)H * W, p = (long long)row * W + x0;
  const long long i0 = (long long)b * 3 * HW + p, i1 = i0 + HW, i2 = i1 + HW;
  if (vec) {                    // W % 4 == 0 and 16-byte aligned pointers: nv = 4 and every address below is 16-byte aligned
    const float4 a0 = osm::ld4(y + i0), a1 = osm::ld4(y + i1), a2 = osm::ld4(y + i2);
    const float4 one = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const float4 k0 = m0 ? osm::ld4(m0 + i0) : one, k1 = m0 ? osm::ld4(m0 + i1) : one, k2 = m0 ? osm::ld4(m0 + i2) : one;
    float4 e0, e1, e2, o0, o1, o2;
    expand_px(G[0], a0.x, a1.x, a2.x, k0.x, k1.x, k2.x, e0.x, e1.x, e2.x, o0.x, o1.x, o2.x);
    expand_px(G[1], a0.y, a1.y, a2.y, k0.y, k1.y, k2.y, e0.y, e1.y, e2.y, o0.y, o1.y, o2.y);
    expand_px(G[2], a0.z, a1.z, a2.z, k0.z, k1.z, k2.z, e0.z, e1.z, e2.z, o0.z, o1.z, o2.z);
    expand_px(G[3], a0.w, a1.w, a2.w, k0.w, k1.w, k2.w, e0.w, e1.w, e2.w, o0.w, o1.w, o2.w);
    osm::st4(ye + i0, e0);
    osm::st4(ye + i1, e1);
    osm::st4(ye + i2, e2);
    osm::st4(me + i0, o0);
    osm::st4(me + i1, o1);
    osm::st4(me + i2, o2);
    osm::st4(field + (long long)b * HW + p, make_float4(G[0], G[1], G[2], G[3]));
    return;
  }
  for (int k = 0; k < nv; ++k) {
    float e0, e1, e2, o0, o1, o2;
    expand_px(G[k], y[i0 + k], y[i1 + k], y[i2 + k], m0 ? m0[i0 + k] : 1.0f, m0 ? m0[i1 + k] : 1.0f, m0 ? m0[i2 + k] : 1.0f, e0, e1, e2,
              o0, o1, o2);
    ye[i0 + k] = e0;
    ye[i1 + k] = e1;
    ye[i2 + k] = e2;
    me[i0 + k] = o0;
    me[i1 + k] = o1;
    me[i2 + k] = o2;
    field[(long long)b * HW + p + k] = G[k];
  }
}

// the first index in [0, n) whose clamped cell index is >= v (n when there is none); tab is non-decreasing
__device__ __forceinline__ int first_ge(const int* __restrict__ tab, int n, int hi, int v) {
  int lo = 0, up = n;
  while (lo < up) {
    const int mid = (lo + up) >> 1;
    if (clampi(tab[mid], hi) >= v) up = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void gain_rows_kernel(const GainTabs tb, const float* __restrict__ nodes, const float* __restrict__ F,
                                                        const float* __restrict__ y, const float* __restrict__ m0, float* __restrict__ t,
                                                        float* __restrict__ s, const int H, const int W, const int gh, const int gw,
                                                        const int P) {
  extern __shared__ float qbuf[];                 // [4][W]: q of the row each wave owns
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave, b = blockIdx.y;
  const bool live = row < H;                      // (wave-uniform; a dead wave only keeps the barrier company)
  float* qr = qbuf + wave * W;
  if (live) {
    const int iy = clampi(tb.iy0[row], gh - 2);
    const float fyv = tb.fy[row], bw = __fsub_rn(1.0f, fyv);
    const float* n0 = nodes + (long long)b * gh * gw + iy * gw;
    const float* n1 = n0 + gw;
    const long long HW = (long long)H * W, p0 = (long long)row * W;
    const float* Fb = F + (long long)b * P * HW + p0;
    const float* yb = y + (long long)b * 3 * HW + p0;
    const float* mb = m0 ? m0 + (long long)b * 3 * HW + p0 : nullptr;
    float sacc = 0.0f;
    for (int x = lane; x < W; x += 64) {
      const float G = gain_at(n0, n1, clampi(tb.ix0[x], gw - 2), tb.fx[x], bw, fyv);
      const float w = P == 4 ? Fb[3 * HW + x] : 1.0f;
      float q = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float f = Fb[c * HW + x], m = mb ? mb[c * HW + x] : 1.0f;
        const float pr = __fsub_rn(__fmul_rn(2.0f, __fmul_rn(G, f)), 1.0f);
        const float r = __fmul_rn(__fmul_rn(__fsub_rn(yb[c * HW + x], pr), w), m);
        const float dd = __fmul_rn(__fmul_rn(__fmul_rn(-2.0f, f), w), m);
        const float rd = __fmul_rn(r, dd);
        q = c == 0 ? rd : __fadd_rn(q, rd);
        sacc = __fadd_rn(sacc, __fmul_rn(r, r));
      }
      qr[x] = q;
    }
    sacc = osm::wave_sum(sacc);
    if (lane == 0) s[(long long)b * H + row] = sacc;
  }
  __syncthreads();
  if (!live || lane >= gw) return;
  // node `lane` of this row: the pixels of cell lane - 1 (weight fx) and then of cell lane (weight 1 - fx), ascending x
  const int lo = first_ge(tb.ix0, W, gw - 2, lane - 1), hi = first_ge(tb.ix0, W, gw - 2, lane + 1);
  float acc = 0.0f;
  for (int x = lo; x < hi; ++x) {
    const float f = tb.fx[x];
    const float wgt = clampi(tb.ix0[x], gw - 2) == lane ? __fsub_rn(1.0f, f) : f;
    acc = __fadd_rn(acc, __fmul_rn(wgt, qr[x]));
  }
  t[((long long)b * H + row) * gw + lane] = acc;
}

__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? b : a); }

__global__ __launch_bounds__(256) void gain_step_kernel(const int* __restrict__ iy0, const float* __restrict__ fy,
                                                        const float* __restrict__ t, const float* __restrict__ s,
                                                        float* __restrict__ nodes, double* __restrict__ cs, const int H, const int W,
                                                        const int gh, const int gw, const int loss_type, const float eta,
                                                        const float lambda, const float g_min) {
  __shared__ float nl[GAIN_MAX_G * GAIN_MAX_G];
  __shared__ double red[256];
  const int b = blockIdx.x, ng = gh * gw, tid = threadIdx.x;
  float* nb = nodes + (long long)b * ng;
  double* cb = cs + (long long)b * (ng + 1);
  for (int i = tid; i < ng; i += 256) nl[i] = nb[i];
  __syncthreads();
  double S = 0.0;                                 // every lane adds the same rows in the same order: no broadcast is needed
  for (int r = 0; r < H; ++r) S += (double)s[(long long)b * H + r];
  if (tid == 0) cb[ng] = S;
  double craw[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    if (j >= ng) continue;
    const int jy = j / gw, jx = j - jy * gw;
    const int lo = first_ge(iy0, H, gh - 2, jy - 1), hi = first_ge(iy0, H, gh - 2, jy + 1);
    double acc = 0.0;
    for (int r = lo; r < hi; ++r) {
      const float f = fy[r];
      const float wgt = clampi(iy0[r], gh - 2) == jy ? __fsub_rn(1.0f, f) : f;
      acc += (double)wgt * (double)t[((long long)b * H + r) * gw + jx];
    }
    craw[k] = acc;
    cb[j] = acc;
  }
  // the guards on S (block-uniform): the nodes stay what they are
  if (!(S - S == 0.0) || (loss_type == 0 && S == 0.0)) return;
  const double gscale = loss_type == 0 ? 1.0 / sqrt(S) : 2.0 / (3.0 * (double)H * (double)W);
  const double e = (double)eta, lam = (double)lambda, gm = (double)g_min;
  double u[4] = {0.0, 0.0, 0.0, 0.0};
  double umax = -1.0;                             // (u >= g_min > 0)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    if (j >= ng) continue;
    const int jy = j / gw, jx = j - jy * gw;
    const double n = (double)nl[j];
    double Ln = 0.0;
    if (jy > 0) Ln += n - (double)nl[j - gw];
    if (jx > 0) Ln += n - (double)nl[j - 1];
    if (jx < gw - 1) Ln += n - (double)nl[j + 1];
    if (jy < gh - 1) Ln += n - (double)nl[j + gw];
    const double v = n - e * (gscale * craw[k] + lam * Ln);
    u[k] = v < gm ? gm : v;
    umax = max_nan(umax, u[k]);
  }
  red[tid] = umax;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = max_nan(red[tid], red[tid + o]);
    __syncthreads();
  }
  umax = red[0];
  if (!(umax - umax == 0.0)) return;              // max(u) is not finite (block-uniform)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = tid + 256 * k;
    if (j >= ng) continue;
    const double nn = u[k] / umax;
    nb[j] = (float)(nn < gm ? gm : nn);
  }
}

int check_desc(const char* what, const osm_gain_desc* d) {
  OSM_REQUIRE(d, "%s: null pointer (the descriptor)", what);
  OSM_REQUIRE(d->B > 0 && d->H >= 2 && d->W >= 2, "%s: bad shape B %d, H %d, W %d", what, d->B, d->H, d->W);
  OSM_REQUIRE(d->B <= 65535 && (long long)d->H * d->W < (1LL << 29), "%s: B %d / H %d x W %d are too many for one launch", what, d->B,
              d->H, d->W);
  OSM_REQUIRE(d->gh >= 2 && d->gw >= 2 && d->gh <= GAIN_MAX_G && d->gw <= GAIN_MAX_G && d->gh <= d->H && d->gw <= d->W,
              "%s: bad grid %d x %d (2 <= gh <= min(H, 32), 2 <= gw <= min(W, 32); H %d, W %d)", what, d->gh, d->gw, d->H, d->W);
  OSM_REQUIRE(d->P == 3 || d->P == 4, "%s: P must be 3 or 4 planes, got %d", what, d->P);
  OSM_REQUIRE(d->loss_type == 0 || d->loss_type == 1, "%s: unknown loss_type %d (0 norm, 1 mse)", what, d->loss_type);
  OSM_REQUIRE(d->eta >= 0.0f && d->eta <= 3.0e38f, "%s: eta must be finite and >= 0, got %g", what, (double)d->eta);
  OSM_REQUIRE(d->lambda >= 0.0f && d->lambda <= 3.0e38f, "%s: lambda must be finite and >= 0, got %g", what, (double)d->lambda);
  OSM_REQUIRE(d->g_min > 0.0f && d->g_min <= 3.0e38f, "%s: g_min must be finite and > 0, got %g", what, (double)d->g_min);
  OSM_REQUIRE(d->n_iter >= 1 && d->n_iter <= 1024, "%s: n_iter must be in [1, 1024], got %d", what, d->n_iter);
  OSM_REQUIRE(d->learn == 0 || d->learn == 1, "%s: learn must be 0 or 1, got %d", what, d->learn);
  return OSM_OK;
}

int check_rows(const char* what, const osm_gain_desc* d) {
  OSM_REQUIRE(d->W <= GAIN_MAX_W, "%s: W %d is wider than the %d pixels the row buffers hold", what, d->W, GAIN_MAX_W);
  return OSM_OK;
}

void launch_expand(const osm_gain_desc* d, const GainTabs& tb, const float* nodes, const float* y, const float* M0, float* ye, float* me,
                   float* field, hipStream_t st) {
  const int vec = d->W % 4 == 0 && osm::aligned16(y) && osm::aligned16(ye) && osm::aligned16(me) && osm::aligned16(field) &&
                  (M0 == nullptr || osm::aligned16(M0));
  const int nq = d->H * ((d->W + 3) / 4);
  hipLaunchKernelGGL(gain_expand_kernel, dim3((nq + 255) / 256, d->B), dim3(256), 0, st, tb, nodes, y, M0, ye, me, field, d->H, d->W, d->gh,
                     d->gw, vec);
}

void launch_rows(const osm_gain_desc* d, const GainTabs& tb, const float* nodes, const float* F, const float* y, const float* M0, float* t,
                 float* s, hipStream_t st) {
  hipLaunchKernelGGL(gain_rows_kernel, dim3((d->H + 3) / 4, d->B), dim3(256), (size_t)4 * d->W * sizeof(float), st, tb, nodes, F, y, M0, t, s,
                     d->H, d->W, d->gh, d->gw, d->P);
}

void launch_step(const osm_gain_desc* d, const GainTabs& tb, const float* t, const float* s, float* nodes, double* cs, hipStream_t st) {
  hipLaunchKernelGGL(gain_step_kernel, dim3(d->B), dim3(256), 0, st, tb.iy0, tb.fy, t, s, nodes, cs, d->H, d->W, d->gh, d->gw, d->loss_type,
                     d->eta, d->lambda, d->g_min);
}

}  // namespace

extern "C" int osm_gain_expand(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx,
                               const float* nodes, const float* y, const float* M0, float* y_eff, float* m_eff, float* field,
                               void* stream) {
  const char* what = "osm_gain_expand";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(iy0 && fy && ix0 && fx, "%s: null pointer (the tables iy0 / fy / ix0 / fx)", what);
  OSM_REQUIRE(nodes && y && y_eff && m_eff && field, "%s: null pointer (nodes / y / y_eff / m_eff / field)", what);
  launch_expand(d, GainTabs{iy0, fy, ix0, fx}, nodes, y, M0, y_eff, m_eff, field, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_gain_rows(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx, const float* nodes,
                             const float* F, const float* y, const float* M0, float* t, float* s, void* stream) {
  const char* what = "osm_gain_rows";
  int rc = check_desc(what, d);
  if (rc) return rc;
  rc = check_rows(what, d);
  if (rc) return rc;
  OSM_REQUIRE(iy0 && fy && ix0 && fx, "%s: null pointer (the tables iy0 / fy / ix0 / fx)", what);
  OSM_REQUIRE(nodes && F && y && t && s, "%s: null pointer (nodes / F / y / t / s)", what);
  launch_rows(d, GainTabs{iy0, fy, ix0, fx}, nodes, F, y, M0, t, s, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_gain_step(const osm_gain_desc* d, const int* iy0, const float* fy, const float* t, const float* s, float* nodes,
                             double* cs, void* stream) {
  const char* what = "osm_gain_step";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(iy0 && fy, "%s: null pointer (the tables iy0 / fy)", what);
  OSM_REQUIRE(t && s && nodes && cs, "%s: null pointer (t / s / nodes / cs)", what);
  launch_step(d, GainTabs{iy0, fy, nullptr, nullptr}, t, s, nodes, cs, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_gain_prepare(const osm_gain_desc* d, const int* iy0, const float* fy, const int* ix0, const float* fx, const float* F,
                                const float* y, const float* M0, float* nodes, float* t, float* s, double* cs, float* y_eff,
                                float* m_eff, float* field, int freeze_phi, void* stream) {
  const char* what = "osm_gain_prepare";
  int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(iy0 && fy && ix0 && fx, "%s: null pointer (the tables iy0 / fy / ix0 / fx)", what);
  OSM_REQUIRE(nodes && y && y_eff && m_eff && field, "%s: null pointer (nodes / y / y_eff / m_eff / field)", what);
  const bool learn = d->learn == 1 && freeze_phi == 0;
  if (learn) {
    rc = check_rows(what, d);
    if (rc) return rc;
    OSM_REQUIRE(F && t && s && cs, "%s: null pointer (F / t / s / cs, which a learning sub-step uses)", what);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const GainTabs tb{iy0, fy, ix0, fx};
  if (learn) {
    for (int it = 0; it < d->n_iter; ++it) {
      launch_rows(d, tb, nodes, F, y, M0, t, s, st);
      launch_step(d, tb, t, s, nodes, cs, st);
    }
  }
  launch_expand(d, tb, nodes, y, M0, y_eff, m_eff, field, st);
  return osm::check_launch(what);
}
