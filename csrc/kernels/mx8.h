// MX-FP8 (OCP MXFP8) block quantization shared by the row quantizer, the weight re-quantizer
// (gemm_mx.hip) and the RMSNorm's side output (elementwise.hip).  A block is 32 consecutive k of one
// row: an e8m0 scale byte E (value 2^(E - 127)) and 32 e4m3 bytes of x / 2^(E - 127), rounded to
// nearest even by v_cvt_scalef32_pk_fp8_f16 (which divides by the power of two of its scale operand).
#pragma once
#include "kcommon.h"

namespace mpk {

// The scale byte of a block whose largest magnitude is amax (finite, >= 0, an f16 value): the
// smallest power of two s with amax / s <= 448 = 1.75 * 2^8, so nothing saturates; 127 for amax = 0.
__device__ __forceinline__ uint32_t mx8_scale_e(float amax) {
  const uint32_t b = __float_as_uint(amax);
  if (b == 0u) return 127u;
  const int e = (int)(b >> 23) - 8 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  return (uint32_t)min(254, max(0, e));
}
// 2^(E - 127) as the conversion's scale operand
__device__ __forceinline__ float mx8_scale_f32(uint32_t e) { return __uint_as_float(e << 23); }

// four f16 -> four e4m3 bytes (element j in byte j) of v / s
__device__ __forceinline__ uint32_t mx8_pack4(half2_t a, half2_t b, float s) {
  typedef short s16x2 __attribute__((ext_vector_type(2)));
  s16x2 r = {0, 0};
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, a, s, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, b, s, true);
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ u32x2 mx8_pack8(half8_t v, float s) {
  return u32x2{mx8_pack4(half2_t{v[0], v[1]}, half2_t{v[2], v[3]}, s), mx8_pack4(half2_t{v[4], v[5]}, half2_t{v[6], v[7]}, s)};
}
__device__ __forceinline__ float amax8(half8_t v) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf((float)v[j]));
  return m;
}

}  // namespace mpk
