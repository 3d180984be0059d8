// Tiled sampling (MultiDiffusion): the data movement between one canvas [C,Hc,Wc] and n overlapping tiles [n,C,th,tw] of the
// network's native size (the engine's x_in / out / d_out / dx layout), and its exact adjoint.
//   gather: tiles[t,c,y,x] = canvas[c, oy_t + y, ox_t + x] k,   k = 1 (plain crop) or wy[y] wx[x] inv_norm[oy_t + y, ox_t + x]
//   blend:  canvas[c,Y,X]  = inv_norm[Y,X] sum_t wy[Y - oy_t] wx[X - ox_t] tiles[t,c,Y - oy_t,X - ox_t]   over the tiles covering (Y, X)
// Both are in gather form: every output element is written by exactly one lane, the blend walks the tiles in ascending index and
// adds in fp32 in that order -- no atomics, so the result does not depend on the launch shape.  A lane owns four consecutive
// elements of an output row: one 16-byte access where the row offset and the base allow it, scalar accesses otherwise (ragged
// origins, a width that is no multiple of 4, the row tail).  Tile origins live on the device; the gather checks them before it
// reads the canvas (a tile whose origin leaves the canvas is written as 0), the blend only ever reads inside a tile.
#include "osm_common.h"

namespace {

constexpr int NT = 256;

struct TileArgs {
  const int* origins;     // [n][2]: (y, x)
  const float* wy;        // [th] or NULL
  const float* wx;        // [tw] or NULL
  const float* inv_norm;  // [Hc][Wc] or NULL
  int n, C, Hc, Wc, th, tw;
};

__global__ __launch_bounds__(NT) void tile_gather_kernel(const float* __restrict__ canvas, float* __restrict__ tiles, const TileArgs a,
                                                         const int aligned) {
  const int vpr = (a.tw + 3) >> 2;                                       // four-element groups per tile row
  const long long total = (long long)a.n * a.C * a.th * vpr;
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % vpr) << 2;
  long long r = i / vpr;
  const int y = (int)(r % a.th);
  r /= a.th;
  const int c = (int)(r % a.C);
  const int t = (int)(r / a.C);
  const int oy = a.origins[2 * t], ox = a.origins[2 * t + 1];
  const bool inside = oy >= 0 && ox >= 0 && oy <= a.Hc - a.th && ox <= a.Wc - a.tw;
  const int nx = min(4, a.tw - x);
  const long long src = ((long long)c * a.Hc + (oy + y)) * a.Wc + ox + x;
  const long long dst = (((long long)t * a.C + c) * a.th + y) * a.tw + x;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (inside) {
    if (aligned && nx == 4 && (src & 3) == 0) {
      const float4 q = osm::ld4(canvas + src);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nx) v[j] = canvas[src + j];
    }
    if (a.wy) {
      const float ky = a.wy[y];
      const long long p = (long long)(oy + y) * a.Wc + ox + x;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nx) v[j] *= (ky * a.wx[x + j]) * a.inv_norm[p + j];
    }
  }
  if (aligned && nx == 4 && (dst & 3) == 0) {
    osm::st4(tiles + dst, make_float4(v[0], v[1], v[2], v[3]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nx) tiles[dst + j] = v[j];
  }
}

__global__ __launch_bounds__(NT) void tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ canvas, const TileArgs a,
                                                        const int aligned) {
#pragma clang fp contract(off)      // weight, product and sum each rounded once, in the stated order
  const int vpr = (a.Wc + 3) >> 2;                                       // four-pixel groups per canvas row
  const long long total = (long long)a.C * a.Hc * vpr;
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int X = (int)(i % vpr) << 2;
  long long r = i / vpr;
  const int Y = (int)(r % a.Hc);
  const int c = (int)(r / a.Hc);
  const int nx = min(4, a.Wc - X);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = 0; t < a.n; ++t) {
    const int oy = a.origins[2 * t], ox = a.origins[2 * t + 1];
    const int y = Y - oy, x = X - ox;                                    // tile-relative position of this lane's first pixel
    if (y < 0 || y >= a.th || x <= -4 || x >= a.tw) continue;
    const long long src = (((long long)t * a.C + c) * a.th + y) * a.tw + x;
    const float ky = a.wy ? a.wy[y] : 1.0f;
    if (aligned && x >= 0 && x + 4 <= a.tw && nx == 4 && (src & 3) == 0) {
      const float4 q = osm::ld4(tiles + src);
      if (a.wy) {
        acc[0] += q.x * (ky * a.wx[x]);
        acc[1] += q.y * (ky * a.wx[x + 1]);
        acc[2] += q.z * (ky * a.wx[x + 2]);
        acc[3] += q.w * (ky * a.wx[x + 3]);
      } else {
        acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nx && x + j >= 0 && x + j < a.tw) {
          const float q = tiles[src + j];
          acc[j] += a.wy ? q * (ky * a.wx[x + j]) : q;
        }
      }
    }
  }
  const long long p = (long long)Y * a.Wc + X;
  const long long dst = (long long)c * a.Hc * a.Wc + p;
  if (a.inv_norm) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nx) acc[j] *= a.inv_norm[p + j];
  }
  if (aligned && nx == 4 && (dst & 3) == 0) {
    osm::st4(canvas + dst, make_float4(acc[0], acc[1], acc[2], acc[3]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nx) canvas[dst + j] = acc[j];
  }
}

int check_args(const char* what, const void* canvas, const void* tiles, const TileArgs& a) {
  OSM_REQUIRE(canvas && tiles && a.origins, "%s: null pointer (canvas / tiles / origins)", what);
  OSM_REQUIRE((a.wy != nullptr) == (a.wx != nullptr) && (a.wy != nullptr) == (a.inv_norm != nullptr),
              "%s: wy, wx and inv_norm are NULL together (plain crop / sum) or all given", what);
  OSM_REQUIRE(a.n >= 1 && a.C >= 1, "%s: bad tile count %d or channel count %d", what, a.n, a.C);
  OSM_REQUIRE(a.Hc >= 1 && a.Wc >= 1 && (long long)a.C * a.Hc * a.Wc < (1LL << 31), "%s: bad canvas %d x %d x %d", what, a.C, a.Hc,
              a.Wc);
  OSM_REQUIRE(a.th >= 1 && a.tw >= 1 && a.th <= a.Hc && a.tw <= a.Wc, "%s: tile %d x %d does not fit the canvas %d x %d", what,
              a.th, a.tw, a.Hc, a.Wc);
  OSM_REQUIRE((long long)a.n * a.C * a.th * ((a.tw + 3) / 4) < (1LL << 31) * NT / 4, "%s: %d tiles of %d x %d x %d are too many", what,
              a.n, a.C, a.th, a.tw);
  return OSM_OK;
}

}  // namespace

extern "C" int osm_tile_gather(const float* canvas, float* tiles, const int* origins, const float* wy, const float* wx,
                               const float* inv_norm, int n, int C, int Hc, int Wc, int th, int tw, void* stream) {
  const TileArgs a{origins, wy, wx, inv_norm, n, C, Hc, Wc, th, tw};
  const int rc = check_args("osm_tile_gather", canvas, tiles, a);
  if (rc != OSM_OK) return rc;
  const long long total = (long long)n * C * th * ((tw + 3) / 4);
  const int aligned = osm::aligned16(canvas) && osm::aligned16(tiles);
  hipLaunchKernelGGL(tile_gather_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, static_cast<hipStream_t>(stream), canvas,
                     tiles, a, aligned);
  return osm::check_launch("osm_tile_gather");
}

extern "C" int osm_tile_blend(const float* tiles, float* canvas, const int* origins, const float* wy, const float* wx,
                              const float* inv_norm, int n, int C, int Hc, int Wc, int th, int tw, void* stream) {
  const TileArgs a{origins, wy, wx, inv_norm, n, C, Hc, Wc, th, tw};
  const int rc = check_args("osm_tile_blend", canvas, tiles, a);
  if (rc != OSM_OK) return rc;
  const long long total = (long long)C * Hc * ((Wc + 3) / 4);
  const int aligned = osm::aligned16(canvas) && osm::aligned16(tiles);
  hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, static_cast<hipStream_t>(stream), tiles,
                     canvas, a, aligned);
  return osm::check_launch("osm_tile_blend");
}
