// Blind deblurring: the gradient of the 'ps' data term with respect to the weights of a point-spread function, and a projected step
// on them (include/osmosis_blind.h).
//   tap gradient   part[b][q][t] = sum over the pixels (i, j) of tile q of r[b,p,i,j] x[b,p, refl_H(i + dy[t]), refl_W(j + dx[t])]
//   step           w <- max(w - eta (g - mean g) - eta l1, 0) / sum,  g[t] = sum_b loss[b] sum_q part[b][q][t] / (3 h w), fp64
// Tap gradient: psf_kernel's tiling (csrc/psf.hip) turned round.  A workgroup owns a TH x TW tile of one plane of one image and stages
// the tile of r and the (TH + 2 Ry) x (TW + 2 Rx) reflected window of x in LDS, rows padded to an odd stride; then every LANE OWNS
// TAPS tid, tid + 256, ... and walks the tile's pixels row-major, one fp32 fma each: the r read is a broadcast (one address for the
// wave), lanes on neighbouring dx read neighbouring window words.  Gather form: every element of `part` is written by exactly one
// lane in a fixed order, no atomics -- the bits depend on neither the batch nor the launch shape.  Lanes idle when T < 256.
// Step: one workgroup per weight set (one set: osm_psf_tap_step; per image / per plane: include/osmosis_psfset.h); the reduction of `part` and everything after it in fp64, sums over t as a strided pass and a halving tree.
#include "osm_common.h"
#include "../../include/osmosis_psf.h"
#include "../../include/osmosis_blind.h"
#include "../../include/osmosis_psfset.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 32;
constexpr int TW = 32;
constexpr int RMAX = 32;                                   // largest halo per side
constexpr int CAP = (TH + 2 * RMAX) * ((TW + 2 * RMAX) | 1);   // 96 x 97 floats (36.4 KB) + the 4 KB tile of r
constexpr int SNT = 1024;                                  // lanes of a step workgroup (one per weight set)

__device__ __forceinline__ int refl(int c, const int n) { return c < 0 ? -c : (c >= n ? 2 * (n - 1) - c : c); }

__global__ __launch_bounds__(NT) void tap_grad_kernel(const float* __restrict__ x, const float* __restrict__ r, const int* __restrict__ dy,
                                                      const int* __restrict__ dx, const int T, const int Ry, const int Rx, const int P,
                                                      const long long xs, const long long rs, const int H, const int W,
                                                      float* __restrict__ part) {
  __shared__ float win[CAP];
  __shared__ __attribute__((aligned(16))) float rt[TH * TW];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TW, i0 = blockIdx.y * TH;
  const int p = (int)(blockIdx.z % P), b = (int)(blockIdx.z / P);
  const int th = min(TH, H - i0), tw = min(TW, W - j0);
  const float* __restrict__ xp = x + (long long)b * xs + (long long)p * H * W;
  const float* __restrict__ rp = r + (long long)b * rs + (long long)p * H * W;
  // the window rows / columns the tile's pixels reach: i0 - Ry .. i0 + th - 1 + Ry (one reflection brings each back: Ry < H)
  const int Hwin = th + 2 * Ry, Wwin = tw + 2 * Rx, LS = (TW + 2 * Rx) | 1;
  for (int wr = tid >> 6; wr < Hwin; wr += NT / 64) {
    const long long row = (long long)refl(i0 - Ry + wr, H) * W;
    for (int wc = tid & 63; wc < Wwin; wc += 64) win[wr * LS + wc] = xp[row + refl(j0 - Rx + wc, W)];
  }
  for (int e = tid; e < TH * TW; e += NT) {
    const int i = e >> 5, j = e & 31;
    rt[e] = (i < th && j < tw) ? rp[(long long)(i0 + i) * W + j0 + j] : 0.0f;
  }
  __syncthreads();
  const long long q = (long long)p * gridDim.x * gridDim.y + (long long)blockIdx.y * gridDim.x + blockIdx.x;
  float* __restrict__ out = part + ((long long)b * P * gridDim.x * gridDim.y + q) * T;
  for (int t = tid; t < T; t += NT) {
    const int dyt = dy[t], dxt = dx[t];
    float acc = 0.0f;
    if (dyt >= -Ry && dyt <= Ry && dxt >= -Rx && dxt <= Rx) {
      const float* __restrict__ base = win + (Ry + dyt) * LS + (Rx + dxt);
      if (tw == TW) {
        for (int i = 0; i < th; ++i) {
#pragma unroll
          for (int j = 0; j < TW; ++j) acc = fmaf(rt[i * TW + j], base[i * LS + j], acc);
        }
      } else {
        for (int i = 0; i < th; ++i)
          for (int j = 0; j < tw; ++j) acc = fmaf(rt[i * TW + j], base[i * LS + j], acc);
      }
    }
    out[t] = acc;
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

// one workgroup per weight set (bi, ci) = blockIdx.x / nc, blockIdx.x % nc: its images b0 .. b1-1 and its partials q0 .. q1-1, ascending
// (one set: all of them -- osm_psf_tap_step's loops)
__global__ __launch_bounds__(SNT) void tap_step_kernel(float* __restrict__ wsets, const float* __restrict__ part, const float* __restrict__ loss,
                                                       const int B, const int nparts, const int T, const double hw3, const double eta,
                                                       const double l1, const int per_image, const int nc, const int ntiles) {
  __shared__ double a[OSM_BLIND_MAX_TAPS];
  __shared__ double red[SNT];
  const int tid = threadIdx.x;
  const int bi = (int)blockIdx.x / nc, ci = (int)blockIdx.x % nc;
  const int b0 = per_image ? bi : 0, b1 = per_image ? bi + 1 : B;
  const int q0 = nc > 1 ? ci * ntiles : 0, q1 = nc > 1 ? q0 + ntiles : nparts;
  float* __restrict__ w = wsets + (long long)blockIdx.x * T;
  for (int t = tid; t < T; t += SNT) {
    double s = 0.0;
    for (int b = b0; b < b1; ++b) {
      const float* __restrict__ pb = part + (long long)b * nparts * T + t;
      double c = 0.0;
      for (int q = q0; q < q1; ++q) c = __dadd_rn(c, (double)pb[(long long)q * T]);
      s = __dadd_rn(s, __dmul_rn((double)loss[b], c));
    }
    a[t] = s / hw3;
  }
  __syncthreads();
  const double gbar = block_sum(a, T, red) / (double)T;
  for (int t = tid; t < T; t += SNT) {                    // (a lane reads and writes its own t only)
    const double v = __dsub_rn(__dsub_rn((double)w[t], __dmul_rn(eta, __dsub_rn(a[t], gbar))), __dmul_rn(eta, l1));
    a[t] = v > 0.0 ? v : 0.0;
  }
  __syncthreads();
  const double S = block_sum(a, T, red);
  if (!(S > 0.0) || isinf(S)) return;                     // every u clamped to 0, or a non-finite loss / gradient: keep the estimate
  for (int t = tid; t < T; t += SNT) w[t] = (float)(a[t] / S);
}

int check_taps(const char* what, const int* dy, const int* dx, int T, int Ry, int Rx, int H, int W) {
  OSM_REQUIRE(dy && dx, "%s: null pointer (a tap array)", what);
  OSM_REQUIRE(T >= 1, "%s: bad tap count T %d", what, T);
  OSM_REQUIRE(H >= 1 && W >= 1 && W <= (1 << 28), "%s: bad image %d x %d", what, H, W);
  OSM_REQUIRE(Ry >= 0 && Rx >= 0 && Ry <= RMAX && Rx <= RMAX, "%s: the radius Ry %d, Rx %d must lie in 0 .. %d (kernels up to %d per side)", what,
              Ry, Rx, RMAX, 2 * RMAX + 1);
  OSM_REQUIRE(Ry < H && Rx < W, "%s: reflection padding needs the radius 0 <= Ry %d < H %d and 0 <= Rx %d < W %d", what, Ry, H, Rx, W);
  return OSM_OK;
}

}  // namespace

extern "C" int osm_psf_tap_grad(const float* x, const float* r, const int* dy, const int* dx, int T, int Ry, int Rx, int B, int P,
                                long long x_img_stride, long long r_img_stride, int H, int W, float* part, void* stream) {
  const char* what = "osm_psf_tap_grad";
  OSM_REQUIRE(x && r && part, "%s: null pointer (x / r / part)", what);
  const int rc = check_taps(what, dy, dx, T, Ry, Rx, H, W);
  if (rc) return rc;
  OSM_REQUIRE(B >= 1 && P >= 1, "%s: bad batch %d or plane count %d", what, B, P);
  OSM_REQUIRE((long long)P * H * W < (1LL << 31), "%s: bad image %d x %d x %d", what, P, H, W);
  OSM_REQUIRE(x_img_stride >= (long long)P * H * W, "%s: x_img_stride %lld is less than the %d planes read", what, x_img_stride, P);
  OSM_REQUIRE(r_img_stride >= (long long)P * H * W, "%s: r_img_stride %lld is less than the %d planes read", what, r_img_stride, P);
  const long long gz = (long long)B * P, gy = (H + TH - 1) / TH;
  OSM_REQUIRE(gz <= 65535 && gy <= 65535, "%s: %lld planes / %lld row tiles are too many for one launch", what, gz, gy);
  hipLaunchKernelGGL(tap_grad_kernel, dim3((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)gz), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, r, dy, dx, T, Ry, Rx, P, x_img_stride, r_img_stride, H, W, part);
  return osm::check_launch(what);
}

namespace {
int check_step(const char* what, int B, int nparts, int T, long long hw3, double eta, double l1) {
  OSM_REQUIRE(B >= 1 && nparts >= 1, "%s: bad batch %d or partial count %d", what, B, nparts);
  OSM_REQUIRE(T >= 1 && T <= OSM_BLIND_MAX_TAPS, "%s: tap count T %d must lie in 1 .. %d", what, T, OSM_BLIND_MAX_TAPS);
  OSM_REQUIRE(hw3 >= 1, "%s: bad normaliser hw3 %lld (3 h w)", what, hw3);
  OSM_REQUIRE(eta == eta && l1 == l1, "%s: eta / l1 is NaN", what);
  return OSM_OK;
}
}  // namespace

extern "C" int osm_psf_tap_step(float* w, const float* part, const float* loss, int B, int nparts, int T, long long hw3, double eta,
                                double l1, void* stream) {
  const char* what = "osm_psf_tap_step";
  OSM_REQUIRE(w && part && loss, "%s: null pointer (w / part / loss)", what);
  const int rc = check_step(what, B, nparts, T, hw3, eta, l1);
  if (rc) return rc;
  hipLaunchKernelGGL(tap_step_kernel, dim3(1), dim3(SNT), 0, static_cast<hipStream_t>(stream), w, part, loss, B, nparts, T, (double)hw3,
                     eta, l1, 0, 1, nparts);
  return osm::check_launch(what);
}

extern "C" int osm_psf_tap_step_s(float* w, const float* part, const float* loss, int B, int P, int ntiles, int T, long long hw3,
                                  double eta, double l1, int per_image, int per_channel, void* stream) {
  const char* what = "osm_psf_tap_step_s";
  OSM_REQUIRE(w && part && loss, "%s: null pointer (w / part / loss)", what);
  OSM_REQUIRE(P >= 1 && ntiles >= 1 && (long long)P * ntiles < (1LL << 31), "%s: bad plane count %d or tile count %d", what, P, ntiles);
  OSM_REQUIRE((per_image == 0 || per_image == 1) && (per_channel == 0 || per_channel == 1), "%s: per_image / per_channel must be 0 or 1, got %d / %d",
              what, per_image, per_channel);
  const int rc = check_step(what, B, P * ntiles, T, hw3, eta, l1);
  if (rc) return rc;
  const int nc = per_channel ? P : 1;
  const long long nsets = (long long)(per_image ? B : 1) * nc;
  OSM_REQUIRE(nsets <= 65535, "%s: %lld weight sets are too many for one launch", what, nsets);
  hipLaunchKernelGGL(tap_step_kernel, dim3((unsigned)nsets), dim3(SNT), 0, static_cast<hipStream_t>(stream), w, part, loss, B, P * ntiles, T,
                     (double)hw3, eta, l1, per_image, nc, ntiles);
  return osm::check_launch(what);
}

namespace {
// osm_ps_blind_optimize (sets = false: the single-set entry points, launch for launch what it was) and osm_ps_blind_optimize_s
int blind_optimize(const char* what, bool sets, const float* x0, const float* y, const float* mask, const int* dy, const int* dx, float* w,
                   int T, int Ry, int Rx, int B, int C, int H, int W, float* Ax, float* r, float* lpart, float* tpart, float* loss,
                   float* g, int n_iter, double eta, double l1, int per_image, int per_channel, void* stream) {
  OSM_REQUIRE(x0 && y && w && Ax && r && lpart && tpart && loss && g, "%s: null pointer", what);
  int rc = check_taps(what, dy, dx, T, Ry, Rx, H, W);
  if (rc) return rc;
  OSM_REQUIRE(B >= 1 && C >= 3, "%s: bad batch %d or channel count %d (the data term reads channels 0..2)", what, B, C);
  OSM_REQUIRE((long long)C * H * W < (1LL << 31) && (long long)H * W < (1 << 29), "%s: bad image %d x %d x %d", what, C, H, W);
  OSM_REQUIRE((long long)B * C <= 65535 && (H + TH - 1) / TH <= 65535, "%s: batch %d x %d planes / %d rows are too many for one launch", what, B,
              C, H);
  OSM_REQUIRE(n_iter >= 1, "%s: n_iter must be >= 1, got %d", what, n_iter);
  OSM_REQUIRE((per_image == 0 || per_image == 1) && (per_channel == 0 || per_channel == 1), "%s: per_image / per_channel must be 0 or 1, got %d / %d",
              what, per_image, per_channel);
  const int HW = H * W;
  const int ntiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  const int nparts = 3 * ntiles;
  rc = check_step(what, B, nparts, T, 3LL * HW, eta, l1);
  if (rc) return rc;
  const long long wp = per_channel ? T : 0, ws = per_image ? (long long)(per_channel ? 3 : 1) * T : 0;
  for (int i = 0; i < n_iter; ++i) {
    rc = sets ? osm_psf_apply_s(x0, Ax, dy, dx, w, T, Ry, Rx, B, 3, (long long)C * HW, 3LL * HW, H, W, 0, 0, ws, wp, stream)
              : osm_psf_apply(x0, Ax, dy, dx, w, T, Ry, Rx, B, 3, (long long)C * HW, 3LL * HW, H, W, 0, 0, stream);
    if (rc) return rc;
    rc = mask ? osm_ps_loss_grad_mc(Ax, y, mask, lpart, loss, r, B, 3, HW, stream) : osm_ps_loss_grad_c(Ax, y, lpart, loss, r, B, 3, HW, stream);
    if (rc) return rc;
    if ((rc = osm_psf_tap_grad(x0, r, dy, dx, T, Ry, Rx, B, 3, (long long)C * HW, 3LL * HW, H, W, tpart, stream))) return rc;
    if (i == n_iter - 1) {
      rc = sets ? osm_psf_apply_s(r, g, dy, dx, w, T, Ry, Rx, B, 3, 3LL * HW, (long long)C * HW, H, W, 1, C - 3, ws, wp, stream)
                : osm_psf_apply(r, g, dy, dx, w, T, Ry, Rx, B, 3, 3LL * HW, (long long)C * HW, H, W, 1, C - 3, stream);
      if (rc) return rc;
    }
    rc = sets ? osm_psf_tap_step_s(w, tpart, loss, B, 3, ntiles, T, 3LL * HW, eta, l1, per_image, per_channel, stream)
              : osm_psf_tap_step(w, tpart, loss, B, nparts, T, 3LL * HW, eta, l1, stream);
    if (rc) return rc;
  }
  return OSM_OK;
}
}  // namespace

extern "C" int osm_ps_blind_optimize(const float* x0, const float* y, const float* mask, const int* dy, const int* dx, float* w, int T,
                                     int Ry, int Rx, int B, int C, int H, int W, float* Ax, float* r, float* lpart, float* tpart,
                                     float* loss, float* g, int n_iter, double eta, double l1, void* stream) {
  return blind_optimize("osm_ps_blind_optimize", false, x0, y, mask, dy, dx, w, T, Ry, Rx, B, C, H, W, Ax, r, lpart, tpart, loss, g, n_iter,
                        eta, l1, 0, 0, stream);
}

extern "C" int osm_ps_blind_optimize_s(const float* x0, const float* y, const float* mask, const int* dy, const int* dx, float* w, int T,
                                       int Ry, int Rx, int B, int C, int H, int W, float* Ax, float* r, float* lpart, float* tpart,
                                       float* loss, float* g, int n_iter, double eta, double l1, int per_image, int per_channel,
                                       void* stream) {
  return blind_optimize("osm_ps_blind_optimize_s", true, x0, y, mask, dy, dx, w, T, Ry, Rx, B, C, H, W, Ax, r, lpart, tpart, loss, g, n_iter,
                        eta, l1, per_image, per_channel, stream);
}
