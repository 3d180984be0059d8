// The operator's depth conversion d = conv_depth(D) of the network's depth plane D, with dd = d d / d D: the ONE definition the
// physics kernels (guidance.hip) and the range-map prior (depthprior.hip) share, so the prior constrains exactly what phi multiplies.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float conv_depth(float D, int type, const float* v, float& dd) {
  if (type == 1) {  // gamma: ((D + v0) * v1) ^ v2
    const float base = (D + v[0]) * v[1];
    if (v[2] == 1.0f) {
      dd = v[1];
      return base;
    }
    const float pw = powf(base, v[2]);
    dd = v[1] * v[2] * powf(base, v[2] - 1.0f);
    return pw;
  }
  if (type == 2) {  // move
    dd = 1.0f;
    return D + v[0];
  }
  dd = 0.5f;  // original
  return 0.5f * (D + 1.0f);
}

}  // namespace
