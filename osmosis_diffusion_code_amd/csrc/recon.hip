// Full-resolution reconstruction: the closed-form inversion of the physical model (osmosis_sampling.py:253-255,287-289)
//   rgb_c = exp(phi_a_c D) (I_c - phi_inf_c (1 - exp(-phi_b_c D))),  D = convert_depth(d)
// evaluated on the ORIGINAL pixel grid: I is the photo before Resize / CenterCrop, d the network's 256-class depth map
// upsampled to that grid, either bilinearly or by joint bilateral upsampling guided by the photo itself (Kopf et al. 2007: a
// spatial Gaussian on the network grid times a range Gaussian between the full-resolution pixel and the low-resolution guide).
//
// One workgroup owns a TW x TH tile of original pixels.  The map from an original pixel to the network grid never upsamples
// by less than 1 (scale <= 1), so the network pixels a tile touches fit a (TH + 2 R) x (TW + 2 R) patch: depth and the three
// guide channels of that patch are staged once in LDS as one float4 per network pixel (one ds_read_b128 per tap).  The
// original image and the outputs are streamed once, 16 bytes per lane and plane where rows are 16-byte aligned.
// The network-grid coordinate v = a i + b is evaluated in double with one rounding per operation, so floor(v) -- which picks
// the window of the joint bilateral filter, a discontinuous choice -- is a well-defined function of the four map numbers.
// No atomics; every output element is written by exactly one lane.
#include "osm_common.h"

namespace {

constexpr int TW = 64;              // tile width (original pixels): 16 lanes x 4 consecutive pixels
constexpr int TH = 16;              // tile height
constexpr int NT = 256;
constexpr int RMAX = 4;
constexpr int PW = TW + 2 * RMAX;   // patch capacity: floor(v_last) - floor(v_first) <= T - 1, plus R - 1 before and R after
constexpr int PH = TH + 2 * RMAX;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// v = a i + b, product and sum rounded separately (no fused multiply-add: hipcc would contract it)
__device__ __forceinline__ double map_coord(double a, double b, int i) {
#pragma clang fp contract(off)
  const double p = a * (double)i;
  return p + b;
}
__device__ __forceinline__ int ifloor(double v) { return (int)floor(fmin(fmax(v, -1.0e6), 1.0e6)); }

__device__ __forceinline__ float convert_depth(float d, int type, const float* v) {
  if (type == 1) {  // gamma: ((d + v0) * v1) ^ v2
    const float base = (d + v[0]) * v[1];
    return v[2] == 1.0f ? base : powf(base, v[2]);
  }
  if (type == 2) return d + v[0];  // move
  return 0.5f * (d + 1.0f);        // original
}

// one axis of a pixel: window origin, fractional offset, and the two bilinear taps (patch-relative indices)
struct Axis {
  int f;        // floor(v)
  float frac;   // v - floor(v)
  int b0, b1;   // bilinear taps of clamp(v, 0, n - 1), patch-relative
  float bw;     // weight of b1
};

__device__ __forceinline__ Axis make_axis(double v, int n, int plo, int phi) {
  Axis a;
  a.f = ifloor(v);
  a.frac = (float)(v - (double)a.f);
  const double vc = fmin(fmax(v, 0.0), (double)(n - 1));
  const int i0 = (int)floor(vc);
  a.bw = (float)(vc - (double)i0);
  a.b0 = clampi(i0, plo, phi) - plo;
  a.b1 = clampi(i0 + 1 < n ? i0 + 1 : n - 1, plo, phi) - plo;
  return a;
}

template <int MODE>
__global__ __launch_bounds__(NT) void recon_kernel(const osm_recon_desc d, const int vec16) {
  __shared__ float4 patch[PH * PW];   // {depth, guide r, g, b} per network pixel
  __shared__ float s_phi[9];          // phi_a[3] | phi_b[3] | phi_inf[3]
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
  const int R = MODE == 0 ? 1 : d.radius;

  // ---- the network pixels this tile touches, clamped to the image (replicate border) and to the patch capacity
  const int Yl = min(Y0 + TH, d.Hc) - 1, Xl = min(X0 + TW, d.Wc) - 1;
  const int py0 = clampi(ifloor(map_coord(d.ay, d.by, Y0)) - R + 1, 0, d.h - 1);
  const int py1 = min(clampi(ifloor(map_coord(d.ay, d.by, Yl)) + R, py0, d.h - 1), py0 + PH - 1);
  const int px0 = clampi(ifloor(map_coord(d.ax, d.bx, X0)) - R + 1, 0, d.w - 1);
  const int px1 = min(clampi(ifloor(map_coord(d.ax, d.bx, Xl)) + R, px0, d.w - 1), px0 + PW - 1);
  const int ph = py1 - py0 + 1, pw = px1 - px0 + 1;
  const int hw = d.h * d.w;
  for (int e = tid; e < ph * pw; e += NT) {
    const int r = e / pw, c = e - r * pw;
    const int gi = (py0 + r) * d.w + px0 + c;
    patch[r * PW + c] = make_float4(d.depth[gi], d.guide[gi], d.guide[hw + gi], d.guide[2 * hw + gi]);
  }
  if (tid < 9) s_phi[tid] = tid < 3 ? d.phi_a[tid] : (tid < 6 ? d.phi_b[tid - 3] : d.phi_inf[tid - 6]);
  __syncthreads();

  const int y = Y0 + ty, x = X0 + 4 * tx;
  if (y >= d.Hc || x >= d.Wc) return;
  const long long plane = (long long)d.Hc * d.Wc;
  const long long o = (long long)y * d.Wc + x;
  const bool vec = vec16 != 0;         // rows 16-byte aligned: Wc % 4 == 0 and aligned bases (then x + 3 < Wc too)
  const int nx = vec ? 4 : min(4, d.Wc - x);

  float I[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (vec) {
      const float4 t = osm::ld4(d.image + c * plane + o);
      I[c][0] = t.x; I[c][1] = t.y; I[c][2] = t.z; I[c][3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) I[c][j] = j < nx ? d.image[c * plane + o + j] : 0.0f;
    }
  }

  const Axis ay = make_axis(map_coord(d.ay, d.by, y), d.h, py0, py1);
  const float cs = 0.5f / (d.sigma_s * d.sigma_s), cr = 0.5f / (d.sigma_r * d.sigma_r);
  float dep[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const Axis ax = make_axis(map_coord(d.ax, d.bx, x + j), d.w, px0, px1);
    const float d00 = patch[ay.b0 * PW + ax.b0].x, d01 = patch[ay.b0 * PW + ax.b1].x;
    const float d10 = patch[ay.b1 * PW + ax.b0].x, d11 = patch[ay.b1 * PW + ax.b1].x;
    const float top = d00 + ax.bw * (d01 - d00), bot = d10 + ax.bw * (d11 - d10);
    float v = top + ay.bw * (bot - top);
    if (MODE == 1) {
      float sw = 0.0f, sd = 0.0f;
      for (int ky = 0; ky < 2 * R; ++ky) {
        const int qy = ay.f - R + 1 + ky;
        const float dy = (float)(ky - R + 1) - ay.frac;
        const int ry = clampi(clampi(qy, 0, d.h - 1), py0, py1) - py0;
        for (int kx = 0; kx < 2 * R; ++kx) {
          const int qx = ax.f - R + 1 + kx;
          const float dx = (float)(kx - R + 1) - ax.frac;
          const int rx = clampi(clampi(qx, 0, d.w - 1), px0, px1) - px0;
          const float4 q = patch[ry * PW + rx];
          const float e0 = I[0][j] - q.y, e1 = I[1][j] - q.z, e2 = I[2][j] - q.w;
          const float wgt = expf(-((dy * dy + dx * dx) * cs + (e0 * e0 + e1 * e1 + e2 * e2) * cr));
          sw += wgt;
          sd += wgt * q.x;
        }
      }
      if (sw > 0.0f) v = sd / sw;   // all weights underflowed: keep the bilinear value
    }
    dep[j] = v;
  }

  float out[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float D = convert_depth(dep[j], d.depth_type, d.dval);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float back = s_phi[6 + c] * (1.0f - expf(-s_phi[3 + c] * D));
      out[c][j] = expf(s_phi[c] * D) * (I[c][j] - back);
    }
  }

  if (vec) {
#pragma unroll
    for (int c = 0; c < 3; ++c) osm::st4(d.rgb + c * plane + o, make_float4(out[c][0], out[c][1], out[c][2], out[c][3]));
    if (d.depth_full) osm::st4(d.depth_full + o, make_float4(dep[0], dep[1], dep[2], dep[3]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nx) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d.rgb[c * plane + o + j] = out[c][j];
        if (d.depth_full) d.depth_full[o + j] = dep[j];
      }
    }
  }
  if (d.rgb_u8) {
    unsigned b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[3 * j + c] = (unsigned)(fminf(fmaxf(out[c][j], 0.0f), 1.0f) * 255.0f);   // truncation
    if (vec) {   // 12 bytes at byte offset 3 o, a multiple of 12
      unsigned* p = reinterpret_cast<unsigned*>(d.rgb_u8 + 3 * o);
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * nx) d.rgb_u8[3 * o + k] = (unsigned char)b[k];
    }
  }
}

}  // namespace

extern "C" int osm_recon_fullres(const osm_recon_desc* d, void* stream) {
  OSM_REQUIRE(d != nullptr, "osm_recon_fullres: null pointer (descriptor)");
  OSM_REQUIRE(d->depth && d->guide && d->image && d->rgb, "osm_recon_fullres: null pointer (depth / guide / image / rgb)");
  OSM_REQUIRE(d->phi_a && d->phi_b && d->phi_inf, "osm_recon_fullres: null pointer (phi_a / phi_b / phi_inf)");
  OSM_REQUIRE(d->h >= 1 && d->w >= 1 && (long long)d->h * d->w <= (1LL << 28), "osm_recon_fullres: bad network grid %d x %d",
              d->h, d->w);
  OSM_REQUIRE(d->Hc >= 1 && d->Wc >= 1 && d->Hc <= 65535 * TH, "osm_recon_fullres: bad rectangle %d x %d", d->Hc, d->Wc);
  OSM_REQUIRE(d->depth_type >= 0 && d->depth_type <= 2, "osm_recon_fullres: unknown depth_type %d", d->depth_type);
  OSM_REQUIRE(d->mode == 0 || d->mode == 1, "osm_recon_fullres: mode must be 0 (bilinear) or 1 (joint bilateral), got %d", d->mode);
  OSM_REQUIRE(d->radius >= 1 && d->radius <= RMAX, "osm_recon_fullres: radius must be in 1..%d, got %d", RMAX, d->radius);
  OSM_REQUIRE(d->sigma_s > 0.0f && d->sigma_r > 0.0f, "osm_recon_fullres: sigma_s and sigma_r must be positive");
  OSM_REQUIRE(d->ay > 0.0 && d->ay <= 1.0 && d->ax > 0.0 && d->ax <= 1.0,
              "osm_recon_fullres: map scale must be in (0, 1] (this path only upsamples), got %g, %g", d->ay, d->ax);
  OSM_REQUIRE(d->by == d->by && d->bx == d->bx && fabs(d->by) < 1.0e6 && fabs(d->bx) < 1.0e6,
              "osm_recon_fullres: map offsets must be finite");
  const int vec = (d->Wc % 4 == 0) && osm::aligned16(d->image) && osm::aligned16(d->rgb) &&
          (!d->depth_full || osm::aligned16(d->depth_full)) && (!d->rgb_u8 || (reinterpret_cast<uintptr_t>(d->rgb_u8) & 3) == 0);
  const dim3 grid((d->Wc + TW - 1) / TW, (d->Hc + TH - 1) / TH);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->mode == 0)
    hipLaunchKernelGGL(recon_kernel<0>, grid, dim3(NT), 0, s, *d, vec);
  else
    hipLaunchKernelGGL(recon_kernel<1>, grid, dim3(NT), 0, s, *d, vec);
  return osm::check_launch("osm_recon_fullres");
}
