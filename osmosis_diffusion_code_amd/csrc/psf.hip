// Point-spread-function operators (motion blur, a measured PSF): a 2-D kernel that does not factor per axis, given as a tap list
// dy[T], dx[T], w[T], applied to each image plane over torch 'reflect' padding, and the exact adjoint (include/osmosis_psf.h):
//   forward  out[b,p,i,j] = sum_t w[t] x[b,p, refl_H(i + dy[t]), refl_W(j + dx[t])]
//   adjoint  g[b,p,r,s]   = sum over the mirrors (a, b) of G(rho_a r, sigma_b s),  G(c, e) = sum_t w[t] vz[c - dy[t], e - dx[t]]
//            (vz: v extended by zeros; rho / sigma: the point itself, its mirror about 0 and about n - 1 -- the transpose of the padding)
// One launch.  A workgroup owns a TH x TW tile of one output plane and runs one PASS per mirror pair (one for the forward, one for an
// interior tile of the adjoint, up to nine at a corner): it stages the (TH + 2 Ry) x (TW + 2 Rx) window of the source the pass
// reads in LDS -- reflection (forward) or zero extension (adjoint) resolved while staging, rows padded to an odd stride so the four
// rows of a 32-lane group fall on different banks -- then every lane walks the tap list for four consecutive outputs of a row: the
// taps are uniform (scalar loads), and a tap that continues the previous one along its row (dx + 1) reuses three of the lane's four
// values and reads one.  A pass whose window misses the image is skipped (it would add +0).
// Gather form: every output element is written by exactly one lane, taps ascending, each one fp32 fma, the passes added in a fixed
// order -- no atomics, the result depends on neither the launch shape nor the batch.  A window larger than the LDS buffer (a halo
// beyond 2 * 32 at a square kernel) is not staged: the lanes take the same values in the same order straight from global memory,
// so the bits do not depend on which way a tile went.  A tap beyond (Ry, Rx) is skipped, never read.
#include "osm_common.h"
#include "../../include/osmosis_psf.h"
#include "../../include/osmosis_psfset.h"

namespace {

constexpr int NT = 256;
constexpr int TH = 32;          // output rows of a tile
constexpr int TW = 32;          // output columns of a tile: NT lanes = TH rows x TW / 4 four-column groups
constexpr int CAP = 96 * 97;    // floats of the LDS window (36.4 KB; four workgroups per CU): k = 61 needs 92 rows of stride 93
static_assert(NT == TH * (TW / 4), "one lane per four consecutive outputs of the tile");

struct PsfArgs {
  const int* dy;
  const int* dx;
  const float* w;
  int T, Ry, Rx, B, P, Z;
  long long xs, os;
  int H, W, adjoint;
  long long ws, wp;       // the weight set of plane (b, p): w + b ws + p wp (include/osmosis_psfset.h; 0, 0: one set for all)
};

// the source element at (r, c) of the extended plane: reflected once (forward) or 0 outside the plane (adjoint; and the forward's
// positions that one reflection does not bring back -- only a lane outside the image asks for those)
__device__ __forceinline__ float src(const float* __restrict__ xp, int r, int c, const int H, const int W, const int adjoint) {
  if (!adjoint) {
    r = r < 0 ? -r : (r >= H ? 2 * (H - 1) - r : r);
    c = c < 0 ? -c : (c >= W ? 2 * (W - 1) - c : c);
  }
  return (r >= 0 && r < H && c >= 0 && c < W) ? xp[(long long)r * W + c] : 0.0f;
}

__global__ __launch_bounds__(NT) void psf_kernel(const float* __restrict__ x, float* __restrict__ out, const PsfArgs a, const int aligned) {
  __shared__ float win[CAP];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TW, i0 = blockIdx.y * TH;
  const int planes = a.P + a.Z;
  const int plane = (int)(blockIdx.z % planes), b = (int)(blockIdx.z / planes);
  const int H = a.H, W = a.W, Ry = a.Ry, Rx = a.Rx;
  const int th = min(TH, H - i0), tw = min(TW, W - j0);
  const int i = tid >> 3, jq = (tid & 7) << 2;                           // this lane's outputs: row i0 + i, columns j0 + jq .. + 3
  const int nx = min(4, tw - jq);
  const bool live = i < th && nx > 0;
  const long long off = (long long)b * a.os + (long long)plane * H * W + (long long)(i0 + i) * W + j0 + jq;
  float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (plane < a.P) {                                                     // (uniform per workgroup, as are `staged` and a skipped pass)
    const float* __restrict__ xp = x + (long long)b * a.xs + (long long)plane * H * W;
    const float* __restrict__ wv = a.w + (long long)b * a.ws + (long long)plane * a.wp;     // uniform: the tap loop's weight loads stay scalar
    const int Hwin = TH + 2 * Ry, Wwin = TW + 2 * Rx, LS = Wwin | 1;
    const bool staged = (long long)Hwin * LS <= CAP;
    const int sd = a.adjoint ? -1 : 1;                                   // the source index moves with (forward) or against a tap's offset
    const int nmir = a.adjoint ? 3 : 1;
    const int r = i0 + i;
    for (int pa = 0; pa < nmir; ++pa) {                                  // rows: the point itself, its mirror about 0, about H - 1
      for (int pb = 0; pb < nmir; ++pb) {                                // columns alike
        const int mr = pa == 1 ? 0 : 2 * (H - 1), mc = pb == 1 ? 0 : 2 * (W - 1);
        const int wr0 = (pa ? mr - (i0 + TH - 1) : i0) - Ry;             // the window's first row / column in the extended plane
        const int wc0 = (pb ? mc - (j0 + TW - 1) : j0) - Rx;
        if (wr0 > H - 1 || wr0 + Hwin - 1 < 0 || wc0 > W - 1 || wc0 + Wwin - 1 < 0) continue;      // all zeros (never the first pass)
        const bool rok = pa == 0 || (pa == 1 ? r >= 1 : r <= H - 2);
        const int cr = pa ? mr - r : r;                                  // this lane's row of G, and its column for k = 0 (k-th: + sk k)
        const int ce0 = pb ? mc - (j0 + jq) : j0 + jq;
        const int sk = pb ? -1 : 1;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (staged) {
          __syncthreads();                                               // the previous pass has read its window
          for (int wr = tid >> 6; wr < Hwin; wr += NT / 64)
            for (int wc = tid & 63; wc < Wwin; wc += 64) win[wr * LS + wc] = src(xp, wr0 + wr, wc0 + wc, H, W, a.adjoint);
          __syncthreads();
          const float* __restrict__ lane = win + (cr - wr0) * LS + (ce0 - wc0);
          const bool same = sk == sd;
          float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          int pdy = 0, pdx = 0;
          bool have = false;
          for (int t = 0; t < a.T; ++t) {
            const int dyt = a.dy[t], dxt = a.dx[t];
            if (dyt < -Ry || dyt > Ry || dxt < -Rx || dxt > Rx) continue;
            const float* __restrict__ p = lane + sd * (dyt * LS + dxt);
            if (have && dyt == pdy && dxt == pdx + 1) {                  // the previous tap's neighbour: every index moved by sd
              if (same) {
                v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = p[3 * sk];
              } else {
                v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = p[0];
              }
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] = p[sk * k];
            }
            have = true; pdy = dyt; pdx = dxt;
            const float wt = wv[t];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fmaf(wt, v[k], acc[k]);
          }
        } else if (live && rok) {
          for (int t = 0; t < a.T; ++t) {
            const int dyt = a.dy[t], dxt = a.dx[t];
            if (dyt < -Ry || dyt > Ry || dxt < -Rx || dxt > Rx) continue;
            const float wt = wv[t];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (k < nx) acc[k] = fmaf(wt, src(xp, cr + sd * dyt, ce0 + sk * k + sd * dxt, H, W, a.adjoint), acc[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int s = j0 + jq + k;
          const bool cok = pb == 0 || (pb == 1 ? s >= 1 : s <= W - 2);
          if (pa == 0 && pb == 0) tot[k] = acc[k];
          else if (rok && cok) tot[k] += acc[k];
        }
      }
    }
  }
  if (!live) return;
  if (aligned && nx == 4 && (off & 3) == 0) {
    osm::st4(out + off, make_float4(tot[0], tot[1], tot[2], tot[3]));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nx) out[off + k] = tot[k];
  }
}

}  // namespace

namespace {
int psf_launch(const char* what, const float* x, float* out, const int* dy, const int* dx, const float* w, int T, int Ry, int Rx, int B,
               int P, long long x_img_stride, long long out_img_stride, int H, int W, int adjoint, int zero_planes, long long ws,
               long long wp, void* stream) {
  OSM_REQUIRE(x && out && dy && dx && w, "%s: null pointer (x / out / a tap array)", what);
  OSM_REQUIRE(B >= 1 && P >= 1 && zero_planes >= 0, "%s: bad batch %d, plane count %d or zero_planes %d", what, B, P, zero_planes);
  OSM_REQUIRE(H >= 1 && W >= 1 && W <= (1 << 28) && ((long long)P + zero_planes) * H * W < (1LL << 31), "%s: bad image %d x %d x %d", what,
              P + zero_planes, H, W);
  OSM_REQUIRE(T >= 1, "%s: bad tap count T %d", what, T);
  OSM_REQUIRE(Ry >= 0 && Rx >= 0 && Ry < H && Rx < W, "%s: reflection padding needs the radius 0 <= Ry %d < H %d and 0 <= Rx %d < W %d", what,
              Ry, H, Rx, W);
  OSM_REQUIRE(adjoint == 0 || adjoint == 1, "%s: adjoint must be 0 or 1, got %d", what, adjoint);
  OSM_REQUIRE(x_img_stride >= (long long)P * H * W, "%s: x_img_stride %lld is less than the %d planes read", what, x_img_stride, P);
  OSM_REQUIRE(out_img_stride >= ((long long)P + zero_planes) * H * W, "%s: out_img_stride %lld is less than the %d planes written", what,
              out_img_stride, P + zero_planes);
  OSM_REQUIRE(ws >= 0 && wp >= 0 && (wp == 0 || wp >= T), "%s: weight strides must be >= 0 and a non-zero w_plane_stride >= T %d, got %lld / %lld",
              what, T, ws, wp);
  OSM_REQUIRE(ws == 0 || ws >= (long long)(P - 1) * wp + T, "%s: w_img_stride %lld does not cover an image's %d planes at w_plane_stride %lld", what,
              ws, P, wp);
  const long long gz = (long long)B * (P + zero_planes);
  const long long gy = (H + TH - 1) / TH;
  OSM_REQUIRE(gz <= 65535 && gy <= 65535, "%s: %lld planes / %lld row tiles are too many for one launch", what, gz, gy);
  const PsfArgs a{dy, dx, w, T, Ry, Rx, B, P, zero_planes, x_img_stride, out_img_stride, H, W, adjoint, ws, wp};
  const int aligned = osm::aligned16(out);
  hipLaunchKernelGGL(psf_kernel, dim3((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)gz), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, out, a, aligned);
  return osm::check_launch(what);
}
}  // namespace

extern "C" int osm_psf_apply(const float* x, float* out, const int* dy, const int* dx, const float* w, int T, int Ry, int Rx, int B,
                             int P, long long x_img_stride, long long out_img_stride, int H, int W, int adjoint, int zero_planes,
                             void* stream) {
  return psf_launch("osm_psf_apply", x, out, dy, dx, w, T, Ry, Rx, B, P, x_img_stride, out_img_stride, H, W, adjoint, zero_planes, 0, 0,
                    stream);
}

extern "C" int osm_psf_apply_s(const float* x, float* out, const int* dy, const int* dx, const float* w, int T, int Ry, int Rx, int B,
                               int P, long long x_img_stride, long long out_img_stride, int H, int W, int adjoint, int zero_planes,
                               long long w_img_stride, long long w_plane_stride, void* stream) {
  return psf_launch("osm_psf_apply_s", x, out, dy, dx, w, T, Ry, Rx, B, P, x_img_stride, out_img_stride, H, W, adjoint, zero_planes,
                    w_img_stride, w_plane_stride, stream);
}
