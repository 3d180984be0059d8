// Separable banded linear operators A = R_h (x) R_w per image plane (gaussian blur with its reflection padding folded in,
// antialiased bicubic / box downsampling) and, with the transposed tables, their exact adjoints (include/osmosis_linop.h):
//   out[b,p,i,j] = sum_a wt_h[i][a] ( sum_c wt_w[j][c] x[b,p,start_h[i]+a,start_w[j]+c] )
// One launch.  A workgroup owns a TH x TW tile of one output plane: it finds the input rows its tile touches, runs the
// horizontal pass for those rows and its TW columns into LDS (x is read through L1 / L2: at 3 x 256^2 fp32 the whole problem is
// L2-resident), then the vertical pass out of LDS, a lane owning four consecutive outputs of a row: one 16-byte store where
// the element offset and the base allow it, scalar stores otherwise (a width that is no multiple of 4, unaligned rows).
// Gather form: every output element is written by exactly one lane, taps are added in ascending order, each one fp32 fma,
// horizontal sum first -- no atomics, the result depends on neither the launch shape nor the batch.  A tile whose row span
// exceeds the LDS buffer (downsampling by more than 7, or a table that is not monotone) computes the same fmas in the same
// order straight from global memory, so the bits do not depend on which way a tile went.
// The tables are device data: a tap outside [0,Hin) x [0,Win) is skipped, never read.
#include "osm_common.h"
#include "../../include/osmosis_linop.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 32;      // output rows of a tile
constexpr int TW = 32;      // output columns of a tile: NT lanes = TH rows x TW / 4 four-column groups
constexpr int RCAP = 256;   // input rows the LDS buffer holds (32 KB): blur k = 61 needs TH + 60 = 92
static_assert(NT == TH * (TW / 4), "one lane per four consecutive outputs of the tile");

struct LinopArgs {
  const int* start_h;
  const float* wt_h;
  const int* start_w;
  const float* wt_w;
  int B, P, Z;
  long long xs, os;
  int Hin, Win, Hout, Wout, Kh, Kw;
};

// sum_c w[c] xrow[s + c], taps ascending, the columns outside the row skipped
__device__ __forceinline__ float hsum(const float* __restrict__ xrow, const float* __restrict__ w, const int s, const int Kw, const int Win) {
  float h = 0.0f;
  for (int c = 0; c < Kw; ++c) {
    const long long col = (long long)s + c;
    if (col >= 0 && col < Win) h = fmaf(w[c], xrow[col], h);
  }
  return h;
}

__global__ __launch_bounds__(NT) void linop_kernel(const float* __restrict__ x, float* __restrict__ out, const LinopArgs a,
                                                   const int aligned) {
  __shared__ __attribute__((aligned(16))) float tmp[RCAP * TW];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TW, i0 = blockIdx.y * TH;
  const int planes = a.P + a.Z;
  const int plane = (int)(blockIdx.z % planes), b = (int)(blockIdx.z / planes);
  const int th = min(TH, a.Hout - i0), tw = min(TW, a.Wout - j0);
  const int i = tid >> 3, jq = (tid & 7) << 2;                           // this lane's outputs: row i0 + i, columns j0 + jq .. + 3
  const int nx = min(4, tw - jq);
  const long long off = (long long)b * a.os + (long long)plane * a.Hout * a.Wout + (long long)(i0 + i) * a.Wout + j0 + jq;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (plane < a.P) {                                                     // (uniform per workgroup, as is `staged`)
    const float* __restrict__ xp = x + (long long)b * a.xs + (long long)plane * a.Hin * a.Win;
    int rmin = a.Hin, rmax = 0;                                          // input rows [rmin, rmax) of this tile, inside the image
    for (int r = 0; r < th; ++r) {
      const long long s = a.start_h[i0 + r];
      rmin = (int)min((long long)rmin, max(s, 0LL));
      rmax = (int)max((long long)rmax, min(s + a.Kh, (long long)a.Hin));
    }
    const int nrows = max(rmax - rmin, 0);
    const bool staged = nrows <= RCAP;
    if (staged) {
      for (int e = tid; e < nrows * TW; e += NT) {
        const int r = e / TW, j = e % TW;
        tmp[e] = j < tw ? hsum(xp + (long long)(rmin + r) * a.Win, a.wt_w + (long long)(j0 + j) * a.Kw, a.start_w[j0 + j], a.Kw, a.Win)
                        : 0.0f;
      }
      __syncthreads();
    }
    if (i < th && nx > 0) {
      const long long s = a.start_h[i0 + i];
      const float* __restrict__ wh = a.wt_h + (long long)(i0 + i) * a.Kh;
      for (int t = 0; t < a.Kh; ++t) {
        const long long r = s + t;
        if (r < rmin || r >= rmax) continue;                             // outside the image
        float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (staged) {
          const float4 q = *reinterpret_cast<const float4*>(&tmp[(int)(r - rmin) * TW + jq]);
          h[0] = q.x; h[1] = q.y; h[2] = q.z; h[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nx) h[k] = hsum(xp + r * a.Win, a.wt_w + (long long)(j0 + jq + k) * a.Kw, a.start_w[j0 + jq + k], a.Kw, a.Win);
        }
        const float w = wh[t];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(w, h[k], acc[k]);
      }
    }
  }
  if (i >= th || nx <= 0) return;
  if (aligned && nx == 4 && (off & 3) == 0) {
    osm::st4(out + off, make_float4(acc[0], acc[1], acc[2], acc[3]));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nx) out[off + k] = acc[k];
  }
}

}  // namespace

extern "C" int osm_linop_apply(const float* x, float* out, const int* start_h, const float* wt_h, const int* start_w,
                               const float* wt_w, int B, int P, long long x_img_stride, long long out_img_stride, int Hin, int Win,
                               int Hout, int Wout, int Kh, int Kw, int zero_planes, void* stream) {
  const char* what = "osm_linop_apply";
  OSM_REQUIRE(x && out && start_h && wt_h && start_w && wt_w, "%s: null pointer (x / out / a table)", what);
  OSM_REQUIRE(B >= 1 && P >= 1 && zero_planes >= 0, "%s: bad batch %d, plane count %d or zero_planes %d", what, B, P, zero_planes);
  OSM_REQUIRE(Hin >= 1 && Win >= 1 && (long long)P * Hin * Win < (1LL << 31), "%s: bad input %d x %d x %d", what, P, Hin, Win);
  OSM_REQUIRE(Hout >= 1 && Wout >= 1 && ((long long)P + zero_planes) * Hout * Wout < (1LL << 31), "%s: bad output %d x %d x %d", what,
              P + zero_planes, Hout, Wout);
  OSM_REQUIRE(Kh >= 1 && Kw >= 1 && (long long)Hout * Kh < (1LL << 31) && (long long)Wout * Kw < (1LL << 31),
              "%s: bad band widths Kh %d, Kw %d", what, Kh, Kw);
  OSM_REQUIRE(x_img_stride >= (long long)P * Hin * Win, "%s: x_img_stride %lld is less than the %d planes read", what, x_img_stride, P);
  OSM_REQUIRE(out_img_stride >= ((long long)P + zero_planes) * Hout * Wout, "%s: out_img_stride %lld is less than the %d planes written",
              what, out_img_stride, P + zero_planes);
  const long long gz = (long long)B * (P + zero_planes);
  const long long gy = (Hout + TH - 1) / TH;
  OSM_REQUIRE(gz <= 65535 && gy <= 65535, "%s: %lld planes / %lld row tiles are too many for one launch", what, gz, gy);
  const LinopArgs a{start_h, wt_h, start_w, wt_w, B, P, zero_planes, x_img_stride, out_img_stride, Hin, Win, Hout, Wout, Kh, Kw};
  const int aligned = osm::aligned16(out);
  hipLaunchKernelGGL(linop_kernel, dim3((unsigned)((Wout + TW - 1) / TW), (unsigned)gy, (unsigned)gz), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, out, a, aligned);
  return osm::check_launch(what);
}
