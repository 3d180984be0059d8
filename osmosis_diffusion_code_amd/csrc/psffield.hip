// Spatially varying blur: a field of point-spread functions on a gh x gw node grid, interpolated bilinearly over the frame
// (include/osmosis_psffield.h, which is the contract).
//   forward  out(p) = b (a c_00 + fx c_01) + fy (a c_10 + fx c_11),  c_kl = the tap-list convolution of csrc/psf.hip at p with the
//            weights of corner (k, l) of p's cell: the OUTPUTS of the four corner PSFs are interpolated, which is the blur with the
//            interpolated kernel because the convolution is linear in its weights
//   adjoint  g = sum over the nodes n, ascending, of A_n (hat_n (.) v),  A_n = psf.hip's adjoint (all mirror passes) with n's weights
// One launch.  A workgroup owns a TH x TW tile of one output plane; a lane owns four consecutive outputs of a row; the taps and
// weights are uniform (scalar loads), a tap that continues the previous one along its row reuses three of the lane's four values.
// Forward: the (TH + 2 Ry) x (TW + 2 Rx) window is staged in LDS ONCE, reflection resolved while staging; the workgroup then walks
// the nodes that are a corner of some pixel of its tile -- [iy0[first row] .. iy0[last row] + 1] x [ix0[first col] .. ix0[last col] + 1]:
// four when the tile lies in one cell, at most nine when the cells are at least a tile wide -- running the tap loop once per node with
// that node's weights; a lane keeps a node's four accumulators as c_kl only where the node is corner (k, l) of its pixel.
// Adjoint: per node whose hat reaches the window of a mirror pass, the window of fl(hat_n v) is staged (zero extension), the taps
// are walked, and the passes, then the nodes, are added in the header's order.  A node / pass that is left out would have added +0.
// A window larger than the LDS buffer is not staged: the lanes take the same values in the same order from global memory.
// Gather form: every output element is written by one lane; no atomics; the bits depend on neither the batch nor the launch shape.
#include <cstdint>
#include "osm_common.h"
#include "../../include/osmosis_psffield.h"

// the hats and the combine: every product and every sum is rounded once, in the order written (the Makefile passes
// -ffp-contract=off as well); the tap loops call fmaf explicitly
#pragma clang fp contract(off)

namespace {

constexpr int MAX_GRID = 32;

constexpr int NT = 256;
constexpr int TH = 32;          // output rows of a tile
constexpr int TW = 32;          // output columns of a tile: NT lanes = TH rows x TW / 4 four-column groups
constexpr int CAP = 96 * 97;    // floats of the LDS window (36.4 KB; four workgroups per CU), as csrc/psf.hip
static_assert(NT == TH * (TW / 4), "one lane per four consecutive outputs of the tile");

struct FieldArgs {
  const int* dy;
  const int* dx;
  const float* w;         // [gh][gw][T]
  int T, Ry, Rx, gh, gw;
  const int* iy0;
  const float* fy;
  const int* ix0;
  const float* fx;
  int B, P, Z;
  long long xs, os;
  int H, W, adjoint;
};

// the cell of position i along an axis with g nodes, clamped into [0, g - 2]
__device__ __forceinline__ int cell(const int* __restrict__ i0, const int i, const int g) { return min(max(i0[i], 0), g - 2); }

// the hat of node j along one axis at position i
__device__ __forceinline__ float hat1(const int* __restrict__ i0, const float* __restrict__ f, const int i, const int j, const int g) {
  const int c = cell(i0, i, g);
  const float fr = f[i];
  return c == j ? 1.0f - fr : (c == j - 1 ? fr : 0.0f);
}

// the source element at (r, c) of the extended plane.  Forward: x reflected once (a position that one reflection does not bring
// back is 0: only a lane outside the image asks for those).  Adjoint: fl(hat_n v) of node n = (ny, nx), 0 outside the plane.
__device__ __forceinline__ float src(const float* __restrict__ xp, int r, int c, const FieldArgs& a, const int ny, const int nx) {
  const int H = a.H, W = a.W;
  if (!a.adjoint) {
    r = r < 0 ? -r : (r >= H ? 2 * (H - 1) - r : r);
    c = c < 0 ? -c : (c >= W ? 2 * (W - 1) - c : c);
  }
  if (!(r >= 0 && r < H && c >= 0 && c < W)) return 0.0f;
  const float v = xp[(long long)r * W + c];
  if (!a.adjoint) return v;
  const float hat = hat1(a.iy0, a.fy, r, ny, a.gh) * hat1(a.ix0, a.fx, c, nx, a.gw);
  return hat * v;
}

// the tap list over a staged window: `lane` is the lane's k = 0 element for a zero offset, its k-th sits sk k further; the source
// index moves with (sd = 1, forward) or against (sd = -1, adjoint) a tap's offset
__device__ __forceinline__ void taps_staged(const float* __restrict__ lane, const int LS, const int sd, const int sk,
                                            const float* __restrict__ wv, const FieldArgs& a, float (&acc)[4]) {
  const bool same = sk == sd;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int pdy = 0, pdx = 0;
  bool have = false;
  for (int t = 0; t < a.T; ++t) {
    const int dyt = a.dy[t], dxt = a.dx[t];
    if (dyt < -a.Ry || dyt > a.Ry || dxt < -a.Rx || dxt > a.Rx) continue;
    const float* __restrict__ p = lane + sd * (dyt * LS + dxt);
    if (have && dyt == pdy && dxt == pdx + 1) {                          // the previous tap's neighbour: every index moved by sd
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
}

// the same values in the same order straight from global memory: the lane's k-th source for a zero offset is (cr, ce0 + sk k)
__device__ __forceinline__ void taps_global(const float* __restrict__ xp, const int cr, const int ce0, const int sd, const int sk,
                                            const int nxl, const float* __restrict__ wv, const FieldArgs& a, const int ny,
                                            const int nx, float (&acc)[4]) {
  for (int t = 0; t < a.T; ++t) {
    const int dyt = a.dy[t], dxt = a.dx[t];
    if (dyt < -a.Ry || dyt > a.Ry || dxt < -a.Rx || dxt > a.Rx) continue;
    const float wt = wv[t];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nxl) acc[k] = fmaf(wt, src(xp, cr + sd * dyt, ce0 + sk * k + sd * dxt, a, ny, nx), acc[k]);
  }
}

__global__ __launch_bounds__(NT) void psf_field_kernel(const float* __restrict__ x, float* __restrict__ out, const FieldArgs a,
                                                       const int aligned) {
  __shared__ float win[CAP];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * TW, i0 = blockIdx.y * TH;
  const int planes = a.P + a.Z;
  const int plane = (int)(blockIdx.z % planes), b = (int)(blockIdx.z / planes);
  const int H = a.H, W = a.W, Ry = a.Ry, Rx = a.Rx, gh = a.gh, gw = a.gw;
  const int th = min(TH, H - i0), tw = min(TW, W - j0);
  const int i = tid >> 3, jq = (tid & 7) << 2;                           // this lane's outputs: row i0 + i, columns j0 + jq .. + 3
  const int nxl = min(4, tw - jq);
  const bool live = i < th && nxl > 0;
  const long long off = (long long)b * a.os + (long long)plane * H * W + (long long)(i0 + i) * W + j0 + jq;
  float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (plane < a.P) {                                                     // (uniform per workgroup, as are `staged`, the node ranges and a skipped pass)
    const float* __restrict__ xp = x + (long long)b * a.xs + (long long)plane * H * W;
    const int Hwin = TH + 2 * Ry, Wwin = TW + 2 * Rx, LS = Wwin | 1;
    const bool staged = (long long)Hwin * LS <= CAP;
    const int r = i0 + i;
    if (!a.adjoint) {
      const int wr0 = i0 - Ry, wc0 = j0 - Rx;
      if (staged) {                                                      // once for every node of the tile
        for (int wr = tid >> 6; wr < Hwin; wr += NT / 64)
          for (int wc = tid & 63; wc < Wwin; wc += 64) win[wr * LS + wc] = src(xp, wr0 + wr, wc0 + wc, a, 0, 0);
        __syncthreads();
      }
      const int rl = min(r, H - 1);                                      // (a lane outside the image reads the tables inside it)
      const int cy = cell(a.iy0, rl, gh);
      int cx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) cx[k] = cell(a.ix0, min(j0 + jq + k, W - 1), gw);
      float c00[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c01[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      float c10[4] = {0.0f, 0.0f, 0.0f, 0.0f}, c11[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      const int ny0 = cell(a.iy0, i0, gh), ny1 = cell(a.iy0, i0 + th - 1, gh) + 1;
      const int nx0 = cell(a.ix0, j0, gw), nx1 = cell(a.ix0, j0 + tw - 1, gw) + 1;
      for (int ny = ny0; ny <= ny1; ++ny) {
        for (int nx = nx0; nx <= nx1; ++nx) {
          const float* __restrict__ wv = a.w + ((long long)ny * gw + nx) * a.T;      // uniform: the weight loads stay scalar
          float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (staged) taps_staged(win + (r - wr0) * LS + (j0 + jq - wc0), LS, 1, 1, wv, a, acc);
          else if (live) taps_global(xp, r, j0 + jq, 1, 1, nxl, wv, a, 0, 0, acc);
          const bool up = ny == cy, dn = ny == cy + 1;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool lf = nx == cx[k], rt = nx == cx[k] + 1;
            if (up && lf) c00[k] = acc[k];
            if (up && rt) c01[k] = acc[k];
            if (dn && lf) c10[k] = acc[k];
            if (dn && rt) c11[k] = acc[k];
          }
        }
      }
      const float fyv = a.fy[rl], bv = 1.0f - fyv;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float fxv = a.fx[min(j0 + jq + k, W - 1)], av = 1.0f - fxv;
        const float p00 = av * c00[k], p01 = fxv * c01[k], p10 = av * c10[k], p11 = fxv * c11[k];
        const float top = p00 + p01, bot = p10 + p11;
        const float q0 = bv * top, q1 = fyv * bot;
        tot[k] = q0 + q1;
      }
    } else {
      // the nodes whose hat reaches a pixel that some pass of this tile reads
      int nyA = gh, nyB = -1, nxA = gw, nxB = -1;
#pragma unroll
      for (int pm = 0; pm < 3; ++pm) {
        const int mr = pm == 1 ? 0 : 2 * (H - 1), mc = pm == 1 ? 0 : 2 * (W - 1);
        const int wr0 = (pm ? mr - (i0 + TH - 1) : i0) - Ry, wc0 = (pm ? mc - (j0 + TW - 1) : j0) - Rx;
        const int rlo = max(wr0, 0), rhi = min(wr0 + Hwin - 1, H - 1), clo = max(wc0, 0), chi = min(wc0 + Wwin - 1, W - 1);
        if (rlo <= rhi) { nyA = min(nyA, cell(a.iy0, rlo, gh)); nyB = max(nyB, cell(a.iy0, rhi, gh) + 1); }
        if (clo <= chi) { nxA = min(nxA, cell(a.ix0, clo, gw)); nxB = max(nxB, cell(a.ix0, chi, gw) + 1); }
      }
      for (int ny = nyA; ny <= nyB; ++ny) {
        for (int nx = nxA; nx <= nxB; ++nx) {
          const float* __restrict__ wv = a.w + ((long long)ny * gw + nx) * a.T;
          float tn[4] = {0.0f, 0.0f, 0.0f, 0.0f};                        // A_n of this node: the passes in psf.hip's order
          for (int pa = 0; pa < 3; ++pa) {                               // rows: the point itself, its mirror about 0, about H - 1
            for (int pb = 0; pb < 3; ++pb) {                             // columns alike
              const int mr = pa == 1 ? 0 : 2 * (H - 1), mc = pb == 1 ? 0 : 2 * (W - 1);
              const int wr0 = (pa ? mr - (i0 + TH - 1) : i0) - Ry;       // the window's first row / column in the extended plane
              const int wc0 = (pb ? mc - (j0 + TW - 1) : j0) - Rx;
              const int rlo = max(wr0, 0), rhi = min(wr0 + Hwin - 1, H - 1), clo = max(wc0, 0), chi = min(wc0 + Wwin - 1, W - 1);
              if (rlo > rhi || clo > chi) continue;                      // the window misses the image: all zeros
              if (ny < cell(a.iy0, rlo, gh) || ny > cell(a.iy0, rhi, gh) + 1 || nx < cell(a.ix0, clo, gw) || nx > cell(a.ix0, chi, gw) + 1)
                continue;                                                // the node's hat misses the window: all zeros
              const bool rok = pa == 0 || (pa == 1 ? r >= 1 : r <= H - 2);
              const int cr = pa ? mr - r : r;                            // this lane's row of G, and its column for k = 0 (k-th: + sk k)
              const int ce0 = pb ? mc - (j0 + jq) : j0 + jq;
              const int sk = pb ? -1 : 1;
              float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
              if (staged) {
                __syncthreads();                                         // the previous pass has read its window
                for (int wr = tid >> 6; wr < Hwin; wr += NT / 64)
                  for (int wc = tid & 63; wc < Wwin; wc += 64) win[wr * LS + wc] = src(xp, wr0 + wr, wc0 + wc, a, ny, nx);
                __syncthreads();
                taps_staged(win + (cr - wr0) * LS + (ce0 - wc0), LS, -1, sk, wv, a, acc);
              } else if (live && rok) {
                taps_global(xp, cr, ce0, -1, sk, nxl, wv, a, ny, nx, acc);
              }
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const int s = j0 + jq + k;
                const bool cok = pb == 0 || (pb == 1 ? s >= 1 : s <= W - 2);
                if (rok && cok) tn[k] = tn[k] + acc[k];
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) tot[k] = tot[k] + tn[k];
        }
      }
    }
  }
  if (!live) return;
  if (aligned && nxl == 4 && (off & 3) == 0) {
    *reinterpret_cast<float4*>(out + off) = make_float4(tot[0], tot[1], tot[2], tot[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nxl) out[off + k] = tot[k];
  }
}

}  // namespace

extern "C" int osm_psf_field_apply(const float* x, float* out, const int* dy, const int* dx, const float* w, int T, int Ry, int Rx,
                                   int gh, int gw, const int* iy0, const float* fy, const int* ix0, const float* fx, int B, int P,
                                   long long x_img_stride, long long out_img_stride, int H, int W, int adjoint, int zero_planes,
                                   void* stream) {
  const char* what = "osm_psf_field_apply";
  OSM_REQUIRE(x && out && dy && dx && w, "%s: null pointer (x / out / a tap array)", what);
  OSM_REQUIRE(iy0 && fy && ix0 && fx, "%s: null pointer (an interpolation table: iy0 / fy / ix0 / fx)", what);
  OSM_REQUIRE(B >= 1 && P >= 1 && zero_planes >= 0, "%s: bad batch %d, plane count %d or zero_planes %d", what, B, P, zero_planes);
  OSM_REQUIRE(H >= 1 && W >= 1 && W <= (1 << 28) && ((long long)P + zero_planes) * H * W < (1LL << 31), "%s: bad image %d x %d x %d", what,
              P + zero_planes, H, W);
  OSM_REQUIRE(gh >= 2 && gw >= 2 && gh <= MAX_GRID && gw <= MAX_GRID && gh <= H && gw <= W,
              "%s: the node grid must be within 2 .. min(%d, the image side) per axis, got %d x %d on a %d x %d image", what, MAX_GRID, gh,
              gw, H, W);
  OSM_REQUIRE(T >= 1, "%s: bad tap count T %d", what, T);
  OSM_REQUIRE(Ry >= 0 && Rx >= 0 && Ry < H && Rx < W, "%s: reflection padding needs the radius 0 <= Ry %d < H %d and 0 <= Rx %d < W %d", what,
              Ry, H, Rx, W);
  OSM_REQUIRE(adjoint == 0 || adjoint == 1, "%s: adjoint must be 0 or 1, got %d", what, adjoint);
  OSM_REQUIRE(x_img_stride >= (long long)P * H * W, "%s: x_img_stride %lld is less than the %d planes read", what, x_img_stride, P);
  OSM_REQUIRE(out_img_stride >= ((long long)P + zero_planes) * H * W, "%s: out_img_stride %lld is less than the %d planes written", what,
              out_img_stride, P + zero_planes);
  const long long gz = (long long)B * (P + zero_planes);
  const long long gy = (H + TH - 1) / TH;
  OSM_REQUIRE(gz <= 65535 && gy <= 65535, "%s: %lld planes / %lld row tiles are too many for one launch", what, gz, gy);
  const FieldArgs a{dy, dx, w, T, Ry, Rx, gh, gw, iy0, fy, ix0, fx, B, P, zero_planes, x_img_stride, out_img_stride, H, W, adjoint};
  const int aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  hipLaunchKernelGGL(psf_field_kernel, dim3((unsigned)((W + TW - 1) / TW), (unsigned)gy, (unsigned)gz), dim3(NT), 0,
                     static_cast<hipStream_t>(stream), x, out, a, aligned);
  return osm::check_launch(what);
}
