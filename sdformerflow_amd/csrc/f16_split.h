// fp32 -> fp16 hi + lo operand split of the fused ANN blocks (ann_block.hip, ann_mlp_block.hip) and their three-product MFMA.
// (dense_linear.hip's split4 and win_attn.hip's split2_f16 are other functions: scalar residuals / another operand layout.)
#pragma once
#include "device_prims.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

// two fp32 -> their hi and lo fp16 halves, packed (win_attn.hip: split2_f16)
__device__ __forceinline__ void split2(float x, float y, uint32_t& hi, uint32_t& lo) {
  const f32x2 v = {x, y};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  const f32x2 r = v - __builtin_convertvector(h, f32x2);
  const f16x2 l = __builtin_convertvector(r, f16x2);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
// eight fp32 -> one hi and one lo operand of v_mfma_f32_16x16x32_f16
__device__ __forceinline__ void split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) split2(x[2 * i], x[2 * i + 1], h[i], l[i]);
  hi = __builtin_bit_cast(f16x8, u32x4{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(f16x8, u32x4{l[0], l[1], l[2], l[3]});
}
// a += A_hi B_hi + A_hi B_lo + A_lo B_hi (the smallest products first)
__device__ __forceinline__ f32x4 mma3(const f16x8& ah, const f16x8& al, const f16x8& bh, const f16x8& bl, f32x4 a) {
  a = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, a, 0, 0, 0);
  a = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, a, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, a, 0, 0, 0);
}

}  // namespace
