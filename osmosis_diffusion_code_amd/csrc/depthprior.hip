// A range-map depth prior in the Osmosis data term (include/osmosis_depthprior.h, which is the contract: the reference has no such
// term).  Per image: six fp64 moments of (m, z, d = conv_depth(D)) over the pixels with m > 0, a closed-form fit d ~ a z + c, the
// loss lambda L of its residual, and the envelope gradient added into the depth plane of g = dL/dx0.  The term does not depend on
// phi, so it runs ONCE per guided sub-step, after the data term's inner loop, whichever route produced g.
//   depth_reduce_kernel  grid (nblk, B) x 256, 1024 pixels per workgroup (phys_reduce_kernel's tiling); fp64 from the first add
//   depth_fit_kernel     one wave per image: the partials, four lanes per component; one lane fits, guards, writes fit / loss
//   depth_grad_kernel    grid (ceil(HW / 256), B): g[b,3,p] += (float)(gs m e dd), nothing else is written
// No atomics, every sum in a fixed order: bit-reproducible, and the bits of an image do not depend on the batch around it.
// Launch- and latency-bound: at most three planes of the image are read (0.8 MB at 256 x 256).
#include "osm_common.h"
#include "depth_conv.h"
#include "../../include/osmosis_depthprior.h"

namespace {

constexpr int PPB = 1024;  // pixels per reduce workgroup
constexpr int NMOM = 6;
constexpr int NSLOT = 8;   // part / tot slots per image (6, 7 are written as 0)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void depth_reduce_kernel(const osm_depth_desc ds, const float* __restrict__ x0,
                                                           const float* __restrict__ z, const float* __restrict__ m,
                                                           double* __restrict__ part, const int nblk) {
  __shared__ double red[4][NSLOT];
  const int b = blockIdx.y, blk = blockIdx.x;
  double s[NMOM];
#pragma unroll
  for (int k = 0; k < NMOM; ++k) s[k] = 0.0;
  const int pend = min(ds.HW, (blk + 1) * PPB);
  const float* __restrict__ Dp = x0 + ((long long)b * 4 + 3) * ds.HW;
  const float* __restrict__ zp = z + (long long)b * ds.HW;
  const float* __restrict__ mp = m + (long long)b * ds.HW;
  for (int p = blk * PPB + threadIdx.x; p < pend; p += 256) {
    const float mf = mp[p];
    if (!(mf > 0.0f)) continue;            // m = 0 (or NaN): nothing of this pixel is used, z may hold anything
    float dd;
    const double d = (double)conv_depth(Dp[p], ds.depth_type, ds.dval, dd);
    const double zz = (double)zp[p], mm = (double)mf;
    const double mz = mm * zz, md = mm * d;
    s[0] += mm;
    s[1] += mz;
    s[2] += md;
    s[3] = fma(mz, zz, s[3]);
    s[4] = fma(mz, d, s[4]);
    s[5] = fma(md, d, s[5]);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NMOM; ++k) {
    const double t = wave_sum_f64(s[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < NSLOT) {
    const int k = threadIdx.x;
    part[((long long)b * nblk + blk) * NSLOT + k] = k < NMOM ? (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]) : 0.0;
  }
}

__global__ __launch_bounds__(64) void depth_fit_kernel(const osm_depth_desc ds, const double* __restrict__ part,
                                                       double* __restrict__ fit, float* __restrict__ depth_loss, const int nblk) {
  __shared__ double tot[NSLOT];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int comp = lane >> 2, sub = lane & 3;     // four lanes share a component's partials (fin_walk's walk); lanes >= 32 idle
  double acc = 0.0;
  if (comp < NSLOT) {
#pragma unroll 4
    for (int k = sub; k < nblk; k += 4) acc += part[((long long)b * nblk + k) * NSLOT + comp];
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (comp < NSLOT && sub == 0) tot[comp] = acc;
  __syncthreads();
  if (lane != 0) return;
  const double Sm = tot[0], Sz = tot[1], Sd = tot[2], Szz = tot[3], Szd = tot[4], Sdd = tot[5];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double two_m40 = 9.094947017729282e-13;   // 2^-40
  double a = ds.align == 0 ? (double)ds.scale : nan, c = ds.align == 0 ? 0.0 : nan, gs = 0.0, L = 0.0;
  bool ok = true;
  if (!(isfinite(Sm) && isfinite(Sz) && isfinite(Sd) && isfinite(Szz) && isfinite(Szd) && isfinite(Sdd))) {
    ok = false;
    L = nan;
  } else if (Sm <= 0.0) {
    ok = false;
  } else if (ds.align == 1) {
    if (Szz <= 0.0) {
      ok = false;
    } else {
      a = fmax(Szd / Szz, (double)ds.scale_min);
      c = 0.0;
    }
  } else if (ds.align == 2) {
    const double det = Sm * Szz - Sz * Sz;
    if (det <= two_m40 * Sm * Szz) {
      ok = false;
    } else {
      a = fmax((Sm * Szd - Sz * Sd) / det, (double)ds.scale_min);
      c = (Sd - a * Sz) / Sm;
    }
  }
  if (ok) {
    const double S = fmax(Sdd - 2.0 * a * Szd - 2.0 * c * Sd + a * a * Szz + 2.0 * a * c * Sz + c * c * Sm, 0.0);
    if (ds.loss_type == 0) {
      if (S <= two_m40 * Sdd) {            // a perfect fit: torch.linalg.norm's backward at 0
        L = 0.0;
        gs = 0.0;
      } else {
        L = sqrt(S);
        gs = (double)ds.lambda / L;
      }
    } else {
      L = S / Sm;
      gs = 2.0 * (double)ds.lambda / Sm;
    }
  }
  fit[b * 4 + 0] = a;
  fit[b * 4 + 1] = c;
  fit[b * 4 + 2] = gs;
  fit[b * 4 + 3] = L;
  depth_loss[b] = (float)L;
}

__global__ __launch_bounds__(256) void depth_grad_kernel(const osm_depth_desc ds, const float* __restrict__ x0,
                                                         const float* __restrict__ z, const float* __restrict__ m,
                                                         const double* __restrict__ fit, float* __restrict__ g) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  const double gs = fit[b * 4 + 2];
  if (!(gs != 0.0) || p >= ds.HW) return;  // a skipped image, a perfect fit or lambda = 0: g is not written
  const float mf = m[(long long)b * ds.HW + p];
  if (!(mf > 0.0f)) return;
  const double a = fit[b * 4 + 0], c = fit[b * 4 + 1];
  const long long ig = ((long long)b * 4 + 3) * ds.HW + p;
  float dd;
  const double d = (double)conv_depth(x0[ig], ds.depth_type, ds.dval, dd);
  const double e = d - (a * (double)z[(long long)b * ds.HW + p] + c);
  const float inc = (float)(gs * (double)mf * e * (double)dd);     // the cast comes before the add: nothing to contract
  g[ig] = g[ig] + inc;
}

int check_desc(const char* what, const osm_depth_desc* d) {
  OSM_REQUIRE(d, "%s: null pointer (the descriptor)", what);
  OSM_REQUIRE(d->align >= 0 && d->align <= 2, "%s: unknown align %d (0 none, 1 scale, 2 affine)", what, d->align);
  OSM_REQUIRE(d->loss_type == 0 || d->loss_type == 1, "%s: unknown loss_type %d (0 norm, 1 mse)", what, d->loss_type);
  OSM_REQUIRE(d->depth_type >= 0 && d->depth_type <= 2, "%s: unknown depth_type %d", what, d->depth_type);
  OSM_REQUIRE(d->lambda >= 0.0f && d->lambda <= 3.0e38f, "%s: lambda must be finite and >= 0, got %g", what, (double)d->lambda);
  OSM_REQUIRE(d->scale >= -3.0e38f && d->scale <= 3.0e38f, "%s: scale must be finite, got %g", what, (double)d->scale);
  OSM_REQUIRE(d->scale_min > 0.0f && d->scale_min <= 3.0e38f, "%s: scale_min must be finite and > 0, got %g", what, (double)d->scale_min);
  OSM_REQUIRE(d->B > 0 && d->HW > 0, "%s: bad shape B %d, HW %d", what, d->B, d->HW);
  OSM_REQUIRE(d->B <= 65535 && d->HW < (1 << 29), "%s: B %d / HW %d are too many for one launch", what, d->B, d->HW);
  return OSM_OK;
}

void launch_reduce(const osm_depth_desc* d, const float* x0, const float* z, const float* m, double* part, hipStream_t st) {
  const int nblk = osm_depth_nblk(d->HW);
  hipLaunchKernelGGL(depth_reduce_kernel, dim3(nblk, d->B), dim3(256), 0, st, *d, x0, z, m, part, nblk);
}

void launch_fit(const osm_depth_desc* d, const double* part, double* fit, float* depth_loss, hipStream_t st) {
  hipLaunchKernelGGL(depth_fit_kernel, dim3(d->B), dim3(64), 0, st, *d, part, fit, depth_loss, osm_depth_nblk(d->HW));
}

void launch_grad(const osm_depth_desc* d, const float* x0, const float* z, const float* m, const double* fit, float* g, hipStream_t st) {
  hipLaunchKernelGGL(depth_grad_kernel, dim3((d->HW + 255) / 256, d->B), dim3(256), 0, st, *d, x0, z, m, fit, g);
}

}  // namespace

extern "C" int osm_depth_nblk(int HW) { return HW > 0 ? (HW + PPB - 1) / PPB : 0; }

extern "C" int osm_depth_reduce(const osm_depth_desc* d, const float* x0, const float* z, const float* m, double* part, void* stream) {
  const char* what = "osm_depth_reduce";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(x0 && z && m && part, "%s: null pointer (x0 / z / m / part)", what);
  launch_reduce(d, x0, z, m, part, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_depth_fit(const osm_depth_desc* d, const double* part, double* fit, float* depth_loss, void* stream) {
  const char* what = "osm_depth_fit";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(part && fit && depth_loss, "%s: null pointer (part / fit / depth_loss)", what);
  launch_fit(d, part, fit, depth_loss, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_depth_grad(const osm_depth_desc* d, const float* x0, const float* z, const float* m, const double* fit, float* g,
                              void* stream) {
  const char* what = "osm_depth_grad";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(x0 && z && m && fit && g, "%s: null pointer (x0 / z / m / fit / g)", what);
  launch_grad(d, x0, z, m, fit, g, static_cast<hipStream_t>(stream));
  return osm::check_launch(what);
}

extern "C" int osm_depth_loss_grad(const osm_depth_desc* d, const float* x0, const float* z, const float* m, double* part, double* fit,
                                   float* depth_loss, float* g, void* stream) {
  const char* what = "osm_depth_loss_grad";
  const int rc = check_desc(what, d);
  if (rc) return rc;
  OSM_REQUIRE(x0 && z && m && part && fit && depth_loss && g, "%s: null pointer (x0 / z / m / part / fit / depth_loss / g)", what);
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_reduce(d, x0, z, m, part, st);
  launch_fit(d, part, fit, depth_loss, st);
  launch_grad(d, x0, z, m, fit, g, st);
  return osm::check_launch(what);
}
