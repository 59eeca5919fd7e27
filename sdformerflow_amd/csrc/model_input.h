// The tail that turns a signed voxel value into the model's input (harness.prepare_chunk; reference eval_DSEC_flow_SNN.py:179-217),
// stated once for prepare_chunk.hip's three entry points and the two voxel front ends (event_voxel.hip, event_voxel_tb.hip): the
// polarity split relu(v) | relu(-v), min / max of the non-zeros, the min-max normalisation, the spike threshold and the event mask.
//
// min / max of the non-zeros are integer atomics on bit patterns: the values are positive floats, which order as their bit patterns, so
// any arrival order gives the same pair.  The pair is kept as {~min, max}: the minimum is the maximum of the complemented pattern, so
// that "no non-zero element" is all-zero for both words and one memset clears every pair of a call.
#pragma once
#include "common.h"

namespace {

// relu as ATen's device clamp_min forms it: NaN stays, else fmaxf(v, 0) = v_max_f32, which orders -0 below +0: relu(-0) = +0
__device__ __forceinline__ float mi_relu(float v) { return v != v ? v : fmaxf(v, 0.f); }

// the polarity split of one signed value: relu(v) | relu(-v) into the pixel's pair of planes (`pair` = the pixel in the first of them,
// the second `hw` elements behind), and the non-zeros into the lane's (~min, max) of bit patterns, which start from (0, 0)
template <typename Index>
__device__ __forceinline__ void mi_split_store(float v, float* __restrict__ pair, Index hw, unsigned& nlo, unsigned& hi) {
  const float o1 = mi_relu(v), o2 = mi_relu(-v);
  pair[0] = o1;
  pair[hw] = o2;
  if (o1 != 0.f) {
    nlo = max(nlo, ~__float_as_uint(o1));
    hi = max(hi, __float_as_uint(o1));
  }
  if (o2 != 0.f) {
    nlo = max(nlo, ~__float_as_uint(o2));
    hi = max(hi, __float_as_uint(o2));
  }
}

__device__ __forceinline__ void mi_wave_minmax(unsigned& nlo, unsigned& hi) {
  for (int off = 32; off > 0; off >>= 1) {
    nlo = max(nlo, (unsigned)__shfl_xor((int)nlo, off));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
  }
}

// the lanes' (~min, max) -> wave -> one pair of atomics on `q` per wave: for a kernel without LDS or a barrier, one value per lane
__device__ __forceinline__ void mi_minmax_commit_wave(unsigned nlo, unsigned hi, unsigned* __restrict__ q) {
  mi_wave_minmax(nlo, hi);
  if ((threadIdx.x & 63) == 0 && hi != 0u) {
    atomicMax(&q[0], nlo);
    atomicMax(&q[1], hi);
  }
}

// the lanes' (~min, max) -> wave -> workgroup (256 threads, every one of them arrives) -> one pair of atomics on `q`: same-address
// atomics serialise in L2, and behind a grid-stride pass a pair per wave cost more than the pass itself
__device__ __forceinline__ void mi_minmax_commit(unsigned nlo, unsigned hi, unsigned* __restrict__ q) {
  mi_wave_minmax(nlo, hi);
  __shared__ unsigned red[4][2];
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = nlo;
    red[threadIdx.x >> 6][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nlo = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
    hi = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    if (hi != 0u) {
      atomicMax(&q[0], nlo);
      atomicMax(&q[1], hi);
    }
  }
}

// prepare_chunk's arithmetic on the values of the split.  mi_norm_of: the pair `q` as {lo, span = hi - lo}; true when there is
// something to normalise: min-max is wanted, the pair holds a non-zero and lo != hi.  mi_finish_value: v <- (v - lo) / span on a
// non-zero when `norm`; then the spike threshold (> th: 1, < th: 0, == th: kept).  The event mask is "any finished value != 0".
// (v by reference: returned by value, prepare_finish_kernel's loop was unrolled to twice the registers.)
__device__ __forceinline__ bool mi_norm_of(const unsigned* q, int want_minmax, float& lo, float& span) {
  bool norm = false;
  lo = 0.f;
  span = 1.f;
  if (want_minmax) {
    const unsigned lob = ~q[0], hib = q[1];
    lo = __uint_as_float(lob);
    span = __uint_as_float(hib) - lo;
    norm = hib != 0u && lob != hib;
  }
  return norm;
}
__device__ __forceinline__ void mi_finish_value(float& v, bool norm, float lo, float span, int want_th, float th) {
  if (norm && v != 0.f) v = (v - lo) / span;
  if (want_th) v = v > th ? 1.f : (v < th ? 0.f : v);
}

// prepare_chunk's tail, one lane per pixel of a sample over its `planes` planes of the split: mi_finish_value in place, and the event mask,
// chunk.sum(1).sum(1).bool(): the values are non-negative here, so their sum is non-zero exactly when one of them is.  The pair is
// mm[2 b] of sample b (per_sample) or mm[0] (the whole batch tensor).  `mul` (the training loop's mask * event_mask; may be NULL):
// (B, 1, h, w) fp32, multiplied by the event mask in place
__global__ __launch_bounds__(256) void prepare_finish_kernel(float* __restrict__ out, float* __restrict__ mask, int64_t pixels, int hw,
                                                             int planes, const unsigned* __restrict__ mm, int want_minmax, int per_sample,
                                                             int want_th, float th, float* __restrict__ mul) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const int64_t b = i / hw;
  float lo, span;
  const bool norm = mi_norm_of(mm + 2 * (per_sample ? b : 0), want_minmax, lo, span);
  float* q = out + b * planes * hw + i % hw;
  bool any = false;
  const bool write = norm || want_th;
  for (int j = 0; j < planes; ++j) {
    float v = q[(int64_t)j * hw];
    mi_finish_value(v, norm, lo, span, want_th, th);
    if (write) q[(int64_t)j * hw] = v;
    any = any || v != 0.f;
  }
  if (mask) mask[i] = any ? 1.f : 0.f;
  if (mul) mul[i] = mul[i] * (any ? 1.f : 0.f);
}

// every pair {~min, max} the call uses: no non-zero element
inline int mi_clear_pairs(unsigned* mm, int pairs, hipStream_t s) { return (int)hipMemsetAsync(mm, 0, (size_t)8 * pairs, s); }

// the launch of prepare_finish_kernel when something is left to do: min-max, threshold, event mask, mask * event mask
inline int mi_finish(float* out, float* event_mask, float* mul, int B, int hw, int planes, const unsigned* mm, int want_minmax,
                     int per_sample, int use_th, float th, hipStream_t s) {
  if (!want_minmax && !use_th && !event_mask && !mul) return 0;
  const int64_t pixels = (int64_t)B * hw;
  SDF_LAUNCH(prepare_finish_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, out, event_mask, pixels, hw, planes, mm,
             want_minmax, per_sample, use_th, th, mul);
  SDF_LAUNCH_CHECK();
  return 0;
}

}  // namespace
