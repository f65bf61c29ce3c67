// IEEE half -> float32 on the device: the one text of the widening that the residency fetch (residency.hip) and K1's
// half-row LOD route (preprocess.hip) share.  Widening is exact, so a value read as a half and widened in registers is
// bit for bit the value a float32 array holding the widened half would have supplied.
#pragma once
#include "common.h"

namespace hgs {

// IEEE half (bits) -> float: exact (v_cvt_f32_f16; subnormal halves become normal floats)
__device__ __forceinline__ float widen_half(uint32_t h) {
  const uint16_t b = (uint16_t)h;
  _Float16 x;
  __builtin_memcpy(&x, &b, 2);
  return (float)x;
}

__device__ __forceinline__ void widen8(const uint4 v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f[2 * t] = widen_half(w[t] & 0xffffu);
    f[2 * t + 1] = widen_half(w[t] >> 16);
  }
}

}  // namespace hgs
