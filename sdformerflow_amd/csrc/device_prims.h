// Device primitives the kernel files share, each stated once: the MFMA accumulator, raw buffer access, the LDS hand-over counters of
// the role-split kernels and the quad transpose.  Includes common.h only and defines no 16-bit matrix-operand type (bf16x8 is `short` x 8
// in spike_mm.h and `__bf16` x 8 in bf16_split.h), so every kernel file may include it.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;   // accumulator of a 16 x 16 MFMA: four fp32 per lane

// Raw buffer access (32-bit byte offset against a wave-uniform descriptor of 2^31 records): an offset with bit 31 set is
// out of range, so the hardware returns zeros for such a load and drops such a store - row / tap / K bounds become an
// offset select instead of an exec-masked branch (hipcc puts a vmcnt wait behind every one of those).
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
constexpr uint32_t INV = 0x80000000u;               // buffer offset of "no such row": loads return zeros, stores are dropped

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)INV, 0x00020000);
}
// the same with a real bound: offsets from `bytes` on are out of range too (the operand's own end, no offset select needed there)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_bounded(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 buf_load16f(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  // (element copies first: __builtin_bit_cast applied directly to a vector-element expression reads element 0 - clang bug)
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  const uint32_t x = v.x, y = v.y, z = v.z, w = v.w;
  return make_float4(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z), __uint_as_float(w));
}
__device__ __forceinline__ void buf_store16f(__amdgpu_buffer_rsrc_t r, uint32_t off, float4 o) {
  u32x4 v;
  v.x = __float_as_uint(o.x); v.y = __float_as_uint(o.y); v.z = __float_as_uint(o.z); v.w = __float_as_uint(o.w);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, 0);
}

// spin until the LDS counter reaches `target` (wave-uniform); later LDS accesses are not hoisted above it
__device__ __forceinline__ void wait_ge(uint32_t* p, uint32_t target) {
  while (true) {
    const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if ((int32_t)(v - target) >= 0) break;
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}
// all LDS operations of this wave have completed -> bump the counter (one lane).  vmcnt is deliberately not waited
// for: the producers' prefetch and the consumers' epilogue stores stay in flight.
__device__ __forceinline__ void signal(uint32_t* p, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// 4 x 4 transpose of dwords among the four lanes of a quad (two DPP butterflies, v_mov_dpp without an `old` operand):
// in: lane q holds a_i = X[q][i]; out: a_i = X[i][q].  o1 / o2 = bit 0 / 1 of the lane's index in its quad.
template <int CTRL>
__device__ __forceinline__ float dpp_quad(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ void qt4(float& a0, float& a1, float& a2, float& a3, bool o1, bool o2) {
  float r = dpp_quad<0xB1>(o1 ? a0 : a1);
  a0 = o1 ? r : a0; a1 = o1 ? a1 : r;
  r = dpp_quad<0xB1>(o1 ? a2 : a3);
  a2 = o1 ? r : a2; a3 = o1 ? a3 : r;
  r = dpp_quad<0x4E>(o2 ? a0 : a2);
  a0 = o2 ? r : a0; a2 = o2 ? a2 : r;
  r = dpp_quad<0x4E>(o2 ? a1 : a3);
  a1 = o2 ? r : a1; a3 = o2 ? a3 : r;
}

}  // namespace
