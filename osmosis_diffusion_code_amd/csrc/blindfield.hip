// Blind spatially varying deblurring: the gradient of the 'ps' data term with respect to the weights of a FIELD of point-spread
// functions, and a projected step of every node (include/osmosis_blindfield.h, which is the contract).
//   tap gradient   part(b, n, p, tile)[t] = sum over the tile's pixels where hat_n is present of fl(hat_n r) x[refl(p + d_t)]
//   step           w_n <- max(w_n - eta (g_n - mean g_n) - eta l1 - eta smooth s_n, 0) / sum,  fp64, s_n the 4-neighbour Laplacian
// Tap gradient: tap_grad_kernel's tiling (csrc/blind.hip).  A workgroup owns a TH x TW tile of one plane of one image and stages the
// tile of r and the reflected window of x in LDS ONCE; then, per node that reaches the tile, it forms the tile of q_n = fl(hat_n r)
// in LDS and every LANE OWNS TAPS tid, tid + 256, ..., walking the rectangle of the tile where the node's hat is present row-major,
// one fp32 fma per pixel: the q read is a broadcast, lanes on neighbouring dx read neighbouring window words.  One node per walk:
// a tile in a cell's interior has four, and a lane's registers hold one accumulator however many reach it.  Gather form: every
// element of `part` is written by exactly one lane in a fixed order, no atomics.
// Step: one workgroup per node reads w (its own and its neighbours') and writes w_new; the entry point copies w_new over w.
#include <cmath>
#include <cstdint>
#include "osm_common.h"
#include "../../include/osmosis_blindfield.h"

// the hats and their product with r: every product is rounded once (the Makefile passes -ffp-contract=off as well); the tap walk
// calls fmaf explicitly, the step uses the __d*_rn intrinsics
#pragma clang fp contract(off)

namespace {

constexpr int MAX_GRID = 32;

constexpr int NT = 256;
constexpr int TH = 32;
constexpr int TW = 32;
constexpr int RMAX = 32;                                       // largest halo per side
constexpr int CAP = (TH + 2 * RMAX) * ((TW + 2 * RMAX) | 1);   // 96 x 97 floats (36.4 KB) + the 4 KB tiles of r and of q_n
constexpr int SNT = 1024;                                      // lanes of a step workgroup (one per node)
constexpr int ABSENT = -4;                                     // the cell of a row / column beyond the image: no node's hat is there

struct GradArgs {
  const int* dy;
  const int* dx;
  int T, Ry, Rx, gh, gw;
  const int* iy0;
  const float* fy;
  const int* ix0;
  const float* fx;
  const int* lay;
  int P;
  long long xs, rs;
  int H, W;
};

__device__ __forceinline__ int refl(int c, const int n) { return c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c); }

__global__ __launch_bounds__(NT) void field_tap_grad_kernel(const float* __restrict__ x, const float* __restrict__ r, const GradArgs a,
                                                            float* __restrict__ part) {
  __shared__ float win[CAP];
  __shared__ __attribute__((aligned(16))) float rt[TH * TW];
  __shared__ __attribute__((aligned(16))) float qt[TH * TW];
  __shared__ int cyT[TH], cxT[TW];                               // the cell of every row / column of the tile
  __shared__ float fyT[TH], fxT[TW];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x, ty = blockIdx.y;
  const int j0 = tx * TW, i0 = ty * TH;
  const int P = a.P, H = a.H, W = a.W, Ry = a.Ry, Rx = a.Rx, T = a.T, gh = a.gh, gw = a.gw;
  const int p = (int)(blockIdx.z % P), b = (int)(blockIdx.z / P);
  const int th = min(TH, H - i0), tw = min(TW, W - j0);
  const float* __restrict__ xp = x + (long long)b * a.xs + (long long)p * H * W;
  const float* __restrict__ rp = r + (long long)b * a.rs + (long long)p * H * W;
  const int Hwin = th + 2 * Ry, Wwin = tw + 2 * Rx, LS = (TW + 2 * Rx) | 1;
  for (int wr = tid >> 6; wr < Hwin; wr += NT / 64) {
    const long long row = (long long)refl(i0 - Ry + wr, H) * W;
    for (int wc = tid & 63; wc < Wwin; wc += 64) win[wr * LS + wc] = xp[row + refl(j0 - Rx + wc, W)];
  }
  for (int e = tid; e < TH * TW; e += NT) {
    const int i = e >> 5, j = e & 31;
    rt[e] = (i < th && j < tw) ? rp[(long long)(i0 + i) * W + j0 + j] : 0.0f;
  }
  if (tid < TH) {
    const bool in = tid < th;
    cyT[tid] = in ? min(max(a.iy0[i0 + tid], 0), gh - 2) : ABSENT;
    fyT[tid] = in ? a.fy[i0 + tid] : 0.0f;
  } else if (tid >= 64 && tid < 64 + TW) {
    const int j = tid - 64;
    const bool in = j < tw;
    cxT[j] = in ? min(max(a.ix0[j0 + j], 0), gw - 2) : ABSENT;
    fxT[j] = in ? a.fx[j0 + j] : 0.0f;
  }
  __syncthreads();
  // the nodes that reach the tile: a corner of the cell of some row and of some column (uniform over the workgroup)
  int ny0 = gh, ny1 = -1, nx0 = gw, nx1 = -1;
  for (int i = 0; i < th; ++i) { ny0 = min(ny0, cyT[i]); ny1 = max(ny1, cyT[i] + 1); }
  for (int j = 0; j < tw; ++j) { nx0 = min(nx0, cxT[j]); nx1 = max(nx1, cxT[j] + 1); }
  const int* __restrict__ lay = a.lay;
  const int* __restrict__ lty0 = lay, * __restrict__ lty1 = lay + gh, * __restrict__ ltx0 = lay + 2 * gh, * __restrict__ ltx1 = lay + 2 * gh + gw;
  const int* __restrict__ loff = lay + 2 * gh + 2 * gw;
  const long long NP = loff[gh * gw];
  for (int ny = ny0; ny <= ny1; ++ny) {
    // the tile rows where the node's row hat is present (an interval for non-decreasing tables; its hull otherwise: q_n is 0 between)
    int ia = TH, ib = -1;
    for (int i = 0; i < th; ++i)
      if (cyT[i] == ny || cyT[i] == ny - 1) { ia = min(ia, i); ib = max(ib, i); }
    if (ib < 0) continue;
    for (int nx = nx0; nx <= nx1; ++nx) {
      int ja = TW, jb = -1;
      for (int j = 0; j < tw; ++j)
        if (cxT[j] == nx || cxT[j] == nx - 1) { ja = min(ja, j); jb = max(jb, j); }
      if (jb < 0) continue;
      // this (node, tile) pair's place in the layout; a pair outside the ranges (tables that are not non-decreasing) is not written
      const int ty0 = lty0[ny], ty1 = lty1[ny], tx0 = ltx0[nx], tx1 = ltx1[nx];
      if (ty < ty0 || ty >= ty1 || tx < tx0 || tx >= tx1) continue;
      const int n = ny * gw + nx;
      const long long slot = (long long)loff[n] + ((long long)p * (ty1 - ty0) + (ty - ty0)) * (tx1 - tx0) + (tx - tx0);
      if (slot < loff[n] || slot >= loff[n + 1] || loff[n + 1] > NP) continue;
      __syncthreads();                                           // the previous node's walk has read qt
      for (int e = tid; e < TH * TW; e += NT) {
        const int i = e >> 5, j = e & 31;
        const int cy = cyT[i], cx = cxT[j];
        float q = 0.0f;
        if ((cy == ny || cy == ny - 1) && (cx == nx || cx == nx - 1)) {
          const float hy = cy == ny ? 1.0f - fyT[i] : fyT[i];
          const float hx = cx == nx ? 1.0f - fxT[j] : fxT[j];
          const float hat = hy * hx;
          q = hat * rt[e];
        }
        qt[e] = q;
      }
      __syncthreads();
      float* __restrict__ out = part + ((long long)b * NP + slot) * T;
      const bool full = ja == 0 && jb == TW - 1;
      for (int t = tid; t < T; t += NT) {
        const int dyt = a.dy[t], dxt = a.dx[t];
        float acc = 0.0f;
        if (dyt >= -Ry && dyt <= Ry && dxt >= -Rx && dxt <= Rx) {
          const float* __restrict__ base = win + (Ry + dyt) * LS + (Rx + dxt);
          if (full) {
            for (int i = ia; i <= ib; ++i) {
#pragma unroll
              for (int j = 0; j < TW; ++j) acc = fmaf(qt[i * TW + j], base[i * LS + j], acc);
            }
          } else {
            for (int i = ia; i <= ib; ++i)
              for (int j = ja; j <= jb; ++j) acc = fmaf(qt[i * TW + j], base[i * LS + j], acc);
          }
        }
        out[t] = acc;
      }
    }
  }
}

// SUM_t of a[0 .. T): lane l sums t = l, l + SNT, ... ascending, then a halving tree over the lanes (the header's order)
__device__ __forceinline__ double block_sum(const double* __restrict__ a, const int T, double* __restrict__ red) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < T; t += SNT) s = __dadd_rn(s, a[t]);
  __syncthreads();                                        // (the previous sum's red[0] has been read)
  red[tid] = s;
  __syncthreads();
  for (int h = SNT / 2; h >= 1; h >>= 1) {
    if (tid < h) red[tid] = __dadd_rn(red[tid], red[tid + h]);
    __syncthreads();
  }
  return red[0];
}

// one workgroup per node n = blockIdx.x
__global__ __launch_bounds__(SNT) void field_tap_step_kernel(const float* __restrict__ w, float* __restrict__ w_new,
                                                             const float* __restrict__ part, const float* __restrict__ loss,
                                                             const int* __restrict__ lay, const int gh, const int gw, const int B,
                                                             const int T, const double hw3, const double eta, const double l1,
                                                             const double smooth) {
  __shared__ double a[OSM_FIELD_MAX_TAPS];
  __shared__ double red[SNT];
  const int tid = threadIdx.x;
  const int n = (int)blockIdx.x, jy = n / gw, jx = n % gw;
  const int* __restrict__ loff = lay + 2 * gh + 2 * gw;
  const long long NP = loff[gh * gw];
  const long long q0 = loff[n], nparts = (long long)loff[n + 1] - q0;
  const float* __restrict__ wn = w + (long long)n * T;
  float* __restrict__ wo = w_new + (long long)n * T;
  for (int t = tid; t < T; t += SNT) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      const float* __restrict__ pb = part + ((long long)b * NP + q0) * T + t;
      double c = 0.0;
      for (long long q = 0; q < nparts; ++q) c = __dadd_rn(c, (double)pb[q * T]);
      s = __dadd_rn(s, __dmul_rn((double)loss[b], c));
    }
    a[t] = s / hw3;
  }
  __syncthreads();
  const double gbar = block_sum(a, T, red) / (double)T;
  const double es = __dmul_rn(eta, smooth);
  for (int t = tid; t < T; t += SNT) {                    // (a lane reads and writes its own t only)
    const double wt = (double)wn[t];
    double v = __dsub_rn(__dsub_rn(wt, __dmul_rn(eta, __dsub_rn(a[t], gbar))), __dmul_rn(eta, l1));
    if (smooth != 0.0) {
      double s = 0.0;
      if (jy > 0) s = __dadd_rn(s, __dsub_rn(wt, (double)wn[t - (long long)gw * T]));
      if (jx > 0) s = __dadd_rn(s, __dsub_rn(wt, (double)wn[t - T]));
      if (jx < gw - 1) s = __dadd_rn(s, __dsub_rn(wt, (double)wn[t + T]));
      if (jy < gh - 1) s = __dadd_rn(s, __dsub_rn(wt, (double)wn[t + (long long)gw * T]));
      v = __dsub_rn(v, __dmul_rn(es, s));
    }
    a[t] = v > 0.0 ? v : 0.0;
  }
  __syncthreads();
  const double S = block_sum(a, T, red);
  const bool ok = S > 0.0 && !isinf(S);                   // else every u clamped to 0, or a non-finite loss / gradient: keep the estimate
  for (int t = tid; t < T; t += SNT) wo[t] = ok ? (float)(a[t] / S) : wn[t];
}

int check_grid(const char* what, int gh, int gw, int H, int W) {
  OSM_REQUIRE(H >= 1 && W >= 1 && W <= (1 << 28), "%s: bad image %d x %d", what, H, W);
  OSM_REQUIRE(gh >= 2 && gw >= 2 && gh <= MAX_GRID && gw <= MAX_GRID && gh <= H && gw <= W,
              "%s: the node grid must be within 2 .. min(%d, the image side) per axis, got %d x %d on a %d x %d image", what, MAX_GRID, gh,
              gw, H, W);
  return OSM_OK;
}

// [first, end) of the 32-wide tiles along one axis of n positions that hold a position whose (clamped) cell is j - 1 or j
void axis_range(const int* i0, int n, int g, int j, int* first, int* end) {
  int lo = -1, hi = -1;
  for (int i = 0; i < n; ++i) {
    int c = i0[i] < 0 ? 0 : (i0[i] > g - 2 ? g - 2 : i0[i]);
    if (c == j || c == j - 1) {
      if (lo < 0) lo = i;
      hi = i;
    }
  }
  *first = lo < 0 ? 0 : lo / 32;
  *end = lo < 0 ? 0 : hi / 32 + 1;
}

}  // namespace

extern "C" long long osm_field_tap_layout(int gh, int gw, const int* iy0, const int* ix0, int H, int W, int P, int B, int T,
                                          int* lay) {
  const char* what = "osm_field_tap_layout";
  OSM_REQUIRE(iy0 && ix0 && lay, "%s: null pointer (iy0 / ix0 / lay)", what);
  if (check_grid(what, gh, gw, H, W)) return OSM_ERR_INVALID;
  OSM_REQUIRE(B >= 1 && P >= 1, "%s: bad batch %d or plane count %d", what, B, P);
  OSM_REQUIRE(T >= 1 && T <= OSM_FIELD_MAX_TAPS, "%s: tap count T %d must lie in 1 .. %d", what, T, OSM_FIELD_MAX_TAPS);
  int* ty0 = lay, * ty1 = lay + gh, * tx0 = lay + 2 * gh, * tx1 = lay + 2 * gh + gw, * off = lay + 2 * gh + 2 * gw;
  for (int jy = 0; jy < gh; ++jy) axis_range(iy0, H, gh, jy, ty0 + jy, ty1 + jy);
  for (int jx = 0; jx < gw; ++jx) axis_range(ix0, W, gw, jx, tx0 + jx, tx1 + jx);
  long long np = 0;
  off[0] = 0;
  for (int jy = 0; jy < gh; ++jy)
    for (int jx = 0; jx < gw; ++jx) {
      np += (long long)P * (ty1[jy] - ty0[jy]) * (tx1[jx] - tx0[jx]);
      OSM_REQUIRE(np < (1LL << 31) / OSM_FIELD_MAX_TAPS, "%s: %lld partials and more are too many", what, np);
      off[jy * gw + jx + 1] = (int)np;
    }
  return (long long)B * np * T;
}

extern "C" int osm_field_tap_grad(const float* x, const float* r, const int* dy, const int* dx, int T, int Ry, int Rx, int gh, int gw,
                                  const int* iy0, const float* fy, const int* ix0, const float* fx, const int* lay, int B, int P,
                                  long long x_img_stride, long long r_img_stride, int H, int W, float* part, void* stream) {
  const char* what = "osm_field_tap_grad";
  OSM_REQUIRE(x && r && part && dy && dx, "%s: null pointer (x / r / part / a tap array)", what);
  OSM_REQUIRE(iy0 && fy && ix0 && fx && lay, "%s: null pointer (an interpolation table: iy0 / fy / ix0 / fx, or the layout)", what);
  if (check_grid(what, gh, gw, H, W)) return OSM_ERR_INVALID;
  OSM_REQUIRE(T >= 1 && T <= OSM_FIELD_MAX_TAPS, "%s: tap count T %d must lie in 1 .. %d", what, T, OSM_FIELD_MAX_TAPS);
  OSM_REQUIRE(Ry >= 0 && Rx >= 0 && Ry <= RMAX && Rx <= RMAX, "%s: the radius Ry %d, Rx %d must lie in 0 .. %d (kernels up to %d per side)",
              what, Ry, Rx, RMAX, 2 * RMAX + 1);
  OSM_REQUIRE(Ry < H && Rx < W, "%s: reflection padding needs the radius 0 <= Ry %d < H %d and 0 <= Rx %d < W %d", what, Ry, H, Rx, W);
  OSM_REQUIRE(B >= 1 && P >= 1, "%s: bad batch %d or plane count %d", what, B, P);
  OSM_REQUIRE((long long)P * H * W < (1LL << 31), "%s: bad image %d x %d x %d", what, P, H, W);
  OSM_REQUIRE(x_img_stride >= (long long)P * H * W, "%s: x_img_stride %lld is less than the %d planes read", what, x_img_stride, P);
  OSM_REQUIRE(r_img_stride >= (long long)P * H * W, "%s: r_img_stride %lld is less than the %d planes read", what, r_img_stride, P);
  const long long gz = (long long)B * P, gy = (H + TH - 1) / TH;
  OSM_REQUIRE(gz <= 65535 && gy <= 65535, "%s: %lld planes / %lld row tiles are too many for one launch", what, gz, gy);
  const GradArgs a{dy, dx, T, Ry, Rx, gh, gw, iy0, fy, ix0, fx, lay, P, x_img_stride, r_img_stride, H, W};
  hipLaunchKernelGGL(field_tap_grad_kernel, dim3((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)gz), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, r, a, part);
  return osm::check_launch(what);
}

extern "C" int osm_field_tap_step(float* w, float* w_new, const float* part, const float* loss, const int* lay, int gh, int gw, int B,
                                  int T, long long hw3, double eta, double l1, double smooth, void* stream) {
  const char* what = "osm_field_tap_step";
  OSM_REQUIRE(w && w_new && part && loss && lay, "%s: null pointer (w / w_new / part / loss / lay)", what);
  OSM_REQUIRE(w != w_new, "%s: w_new must not alias w (a node reads its neighbours while they step)", what);
  OSM_REQUIRE(gh >= 2 && gw >= 2 && gh <= MAX_GRID && gw <= MAX_GRID, "%s: the node grid must be within 2 .. %d per axis, got %d x %d", what,
              MAX_GRID, gh, gw);
  OSM_REQUIRE(B >= 1, "%s: bad batch %d", what, B);
  OSM_REQUIRE(T >= 1 && T <= OSM_FIELD_MAX_TAPS, "%s: tap count T %d must lie in 1 .. %d", what, T, OSM_FIELD_MAX_TAPS);
  OSM_REQUIRE(hw3 >= 1, "%s: bad normaliser hw3 %lld (3 h w)", what, hw3);
  OSM_REQUIRE(eta == eta && l1 == l1, "%s: eta / l1 is NaN", what);
  OSM_REQUIRE(smooth >= 0.0 && !std::isinf(smooth), "%s: smooth must be >= 0 and finite, got %g", what, smooth);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(field_tap_step_kernel, dim3((unsigned)(gh * gw)), dim3(SNT), 0, s, w, w_new, part, loss, lay, gh, gw, B, T, (double)hw3,
                     eta, l1, smooth);
  if (const int rc = osm::check_launch(what)) return rc;
  const hipError_t e = hipMemcpyAsync(w, w_new, sizeof(float) * (size_t)gh * gw * T, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return osm::fail(OSM_ERR_LAUNCH, "%s: copying w_new over w: %s", what, hipGetErrorString(e));
  return OSM_OK;
}
