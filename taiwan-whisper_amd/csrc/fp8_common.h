// What the two e4m3 quantisers share (xkv_fp8.hip: the cross-attention K/V blocks; gemv_w8.hip: the decoder weight
// rows): the hardware conversion, the 16-bit words of a 16-B load as fp32, and the scale exponent of a block.
#pragma once
#include "common.h"

namespace tw8 {

// RNE of y (|y| <= 448 or NaN) to e4m3fn by the hardware conversion: two values into one half of a dword
__device__ __forceinline__ uint32_t cvt4_e4m3(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

// 8 consecutive 16-bit words (one 16-B load) as fp32
template <bool H>
__device__ __forceinline__ void words_f32(const bf16x8 v, float* o) {
  if constexpr (H) {
    const f16x8 h = __builtin_bit_cast(f16x8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)h[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf2f(v[j]);
  }
}

// scale exponent of a block from the fp32 bits of its absmax (finite, > 0): absmax = m * 2^x, m in [0.5, 1);
// e = x - 9 when m <= 0.875 (then absmax * 2^-e <= 0.875 * 512 = 448), else x - 8; fp32 subnormals sit far
// below the clamp
__device__ __forceinline__ int scale_exp(uint32_t u) {
  const int ef = (int)(u >> 23);
  if (ef == 0) return -100;
  const int x = ef - 126;
  const int e = (u & 0x7fffffu) <= 0x600000u ? x - 9 : x - 8;
  return max(-100, min(100, e));
}

}  // namespace tw8
