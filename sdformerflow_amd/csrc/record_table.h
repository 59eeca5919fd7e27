// Per-sample fp64 records without float atomics, stated once for flow_metrics.hip, event_iwe.hip's statistics and event_voxel_tb.hip's
// list statistics: a lane's values -> wave (xor butterfly) -> workgroup (the four waves in a fixed order) -> one partial record of F
// fields per workgroup, and a finish that combines a sample's partial records in index order.  A field is a sum or, where its bit of
// MAXES is set, a maximum.  A record depends on its sample alone: two runs, or two batchings, give the same bits.
#pragma once
#include "common.h"
#include <initializer_list>

namespace {

constexpr int kRtThreads = 256;
constexpr int kRtPerLane = 4;                           // pixels per lane, kRtThreads apart (coalesced)
constexpr int kRtTile = kRtThreads * kRtPerLane;        // pixels per workgroup

// tiles per sample of a (B, ., H, W) image; 0 = refused geometry
inline int64_t rt_tiles(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1) return 0;
  const int64_t hw = (int64_t)H * W;
  if (hw >= (1ll << 30)) return 0;                       // pixel indices and 2 hw stay inside 31 bits
  return (hw + kRtTile - 1) / kRtTile;
}

// a lane's value over its wave; counters stay the integers they are
template <typename T>
__device__ __forceinline__ T rt_wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double rt_wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// the waves' fields `v` (256 threads, every one of them arrives) -> rec[0 .. F): ((w0 + w1) + w2) + w3, a maximum likewise in pairs
template <int F, unsigned MAXES = 0>
__device__ __forceinline__ void rt_block_store(const double (&v)[F], double* __restrict__ rec) {
  __shared__ double red[kRtThreads / 64][F];
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < F; ++k) red[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < F) {
    const int k = threadIdx.x;
    rec[k] = (MAXES >> k) & 1 ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                              : ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// field k of a sample's `nblk` partial records of F fields at `part`, combined in index order from 0
template <int F, unsigned MAXES = 0>
__device__ __forceinline__ double rt_finish_field(const double* __restrict__ part, int nblk, int k) {
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) {
    const double v = part[(int64_t)i * F + k];
    s = (MAXES >> k) & 1 ? fmax(s, v) : s + v;
  }
  return s;
}

// The checks of a call that writes rows row0 .. row0 + B - 1 of a caller's (rows, F) table from (B, ., H, W) images, in the family's
// order behind the NULL descriptor: geometry | rows inside the table | NULL | workspace size | alignment.  `inputs`: the fp32 images,
// all required.  0 and the tiles per sample, or the error.
inline int rt_check(int B, int H, int W, int row0, int rows, int F, std::initializer_list<const void*> inputs, const double* table,
                    const void* workspace, int64_t workspace_bytes, int64_t& tiles) {
  tiles = rt_tiles(B, H, W);
  if (!tiles) return SDF_E_SHAPE;
  if (row0 < 0 || (int64_t)row0 + B > rows) return SDF_E_SHAPE;        // the records lie inside the table
  for (const void* p : inputs)
    if (!p) return SDF_E_NULL;
  if (!table || !workspace) return SDF_E_NULL;
  if (workspace_bytes < (int64_t)B * tiles * F * 8) return SDF_E_SHAPE;
  for (const void* p : inputs)
    if (!sdf_aligned(p, 4)) return SDF_E_ALIGN;
  if (!sdf_aligned(table, 8) || !sdf_aligned(workspace, 8)) return SDF_E_ALIGN;
  return 0;
}

}  // namespace
