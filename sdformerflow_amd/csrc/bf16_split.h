// fp32 -> bf16 hi + mid + lo plane split of the training products (linear_dw.hip, linear_train.hip) and the transposing LDS read
// of their [reduction][column] images.  bf16x8 is `__bf16` x 8 here (the bf16 MFMA builtins' operand type); spike_mm.h's bf16x8 is
// `short` x 8, so a file includes one of the two headers, never both.
#pragma once
#include "device_prims.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// two fp32 values -> the dword {bf16(a), bf16(b)} of their top halves
__device__ __forceinline__ uint32_t top2(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
__device__ __forceinline__ uint2 top4(u32x4 v) { return make_uint2(top2(v.x, v.y), top2(v.z, v.w)); }

// four fp32 values -> three 8-byte words of bf16 planes, hi + mid + lo == v exactly (truncation splits)
__device__ __forceinline__ void split3(u32x4 v, uint2& hi, uint2& mid, uint2& lo) {
  uint32_t h[4], m[4], l[4];
  const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = x[i] & 0xFFFF0000u;
    const float r1 = __uint_as_float(x[i]) - __uint_as_float(h[i]);
    m[i] = __float_as_uint(r1) & 0xFFFF0000u;
    l[i] = __float_as_uint(r1 - __uint_as_float(m[i]));            // <= 8 significant bits: its top half is all of it
  }
  hi = make_uint2(top2(h[0], h[1]), top2(h[2], h[3]));
  mid = make_uint2(top2(m[0], m[1]), top2(m[2], m[3]));
  lo = make_uint2(top2(l[0], l[1]), top2(l[2], l[3]));
}

// reduction indices 4g..4g+3 | 16+4g..16+4g+3 of 16 COLUMNS of a [reduction][column] LDS image of row pitch RP bytes, through the
// transposing read: rows 4g + q (this read) and 16 + 4g + q (the next); element j of the lane = reduction index 4g + j, 16 + 4g + (j - 4)
template <int RP>
__device__ __forceinline__ bf16x8 tr_frag(const uint8_t* p) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 16 * RP));
  s16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
  return __builtin_bit_cast(bf16x8, r);
}

}  // namespace
