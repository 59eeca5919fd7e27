// fp32 membranes -> per-time-step statistics in 64-bit integers (NaN count, fixed-point sum, extremes as ordered keys, histogram), gfx950.
//
// spike_count.hip's sibling on fp32: what a reader of the reference's `v_seq_monitor.records` (eval_DSEC_flow_SNN.py:145-149, 228-230,
// `vis.monitor_v`) looks at, per neuron call and time step, without keeping the membrane.  The record of step t,
//   [n_nan, sum_q16, min_key, max_key, hist[0 .. bins + 1]]        (include/sdformerflow_hip.h SdfMembraneStatsDesc)
// is ADDED to, so one table holds every call of every forward and is read back once.  Integer atomics only - adds, and min / max of
// the order-preserving key of the fp32 bits - are order-independent: the same bits on every run, restated exactly in numpy
// (sdformerflow_amd/monitor.py membrane_record).  Compiled with -ffp-contract=off: the histogram index's subtraction, product and
// floor are rounded one by one.
//
// Two kernels, spike_count.hip's geometry (element (o, t, r, c) at v + ((o T + t) rows + r) row_stride + c, in floats):
//   run   row_stride == C: every (o, t) is ONE run of rows * C floats.  16 bytes per lane from the first 16-byte boundary inside the
//         run; the up to 3 floats in front of it and behind the last whole vector are read one by one by the run's first workgroup, so
//         that nothing outside [base, base + run) is touched whatever the base's alignment.
//   rows  row_stride > C (channel slices: small tensors): element i of an (o, t) block is float i % C of row i / C.
// Both: histogram per workgroup in LDS, flushed with one 64-bit atomic per non-zero slot; NaN count, sum and extremes lane -> wave ->
// workgroup, then one 64-bit atomic each.
#include "common.h"

namespace {

constexpr int kMsThreads = 256;
constexpr int kMsVecs = 8;                                  // 16-byte loads per lane
constexpr int kMsTileVecs = kMsThreads * kMsVecs;           // per workgroup: 2 048 vectors = 32 KiB of a run
constexpr int kMsElems = 32;                                // rows kernel: floats per lane
constexpr int kMsTileElems = kMsThreads * kMsElems;
constexpr int kMsMaxBins = 256;

// Overflow bounds of the partials.  A lane takes at most kMsVecs * 4 + 1 = 33 floats (run kernel: its vectors and one head or tail
// float) or kMsElems = 32 (rows kernel); a workgroup at most 256 * 33 = 8 448.  The 32-bit partials - the lane's and the workgroup's NaN
// count and every LDS histogram slot - are counts of elements, so < 2^14.  |q16| <= 32768 * 65536 = 2^31 does NOT fit 32 bits signed:
// the sum is 64-bit from the lane on, |lane sum| <= 33 * 2^31 < 2^37, |workgroup sum| < 2^45.  The keys are 32-bit values; they are
// widened at the atomic, where the table's slots hold 2^32 - 1 / 0 before the first call.
struct MsLane {
  unsigned nan = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
  long long sum = 0;
};

struct MsBins {
  int bins;
  float lo, hi, inv_width;
};

__device__ __forceinline__ void ms_take(MsLane& L, unsigned* hist, const MsBins& B, float x) {
  if (x != x) {
    ++L.nan;
    return;
  }
  L.sum += (long long)rintf(fminf(fmaxf(x, -32768.f), 32768.f) * 65536.f);
  const unsigned bits = __float_as_uint(x);
  const unsigned key = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  L.kmin = min(L.kmin, key);
  L.kmax = max(L.kmax, key);
  int i;
  if (x < B.lo) {
    i = 0;
  } else if (x >= B.hi) {
    i = B.bins + 1;
  } else {
    const float d = x - B.lo;
    const float p = d * B.inv_width;
    i = 1 + min(B.bins - 1, (int)floorf(p));
  }
  atomicAdd(hist + i, 1u);
}

__device__ __forceinline__ void ms_hist_clear(unsigned* hist, int bins) {
  for (int i = threadIdx.x; i < bins + 2; i += kMsThreads) hist[i] = 0u;
  __syncthreads();
}

// the workgroup's partials into the record `rec` = table + t * (4 + bins + 2)
__device__ __forceinline__ void ms_workgroup_flush(MsLane L, const unsigned* hist, int bins, unsigned long long* rec) {
  for (int off = 32; off > 0; off >>= 1) {
    L.nan += (unsigned)__shfl_xor((int)L.nan, off);
    L.sum += __shfl_xor(L.sum, off);
    L.kmin = min(L.kmin, (unsigned)__shfl_xor((int)L.kmin, off));
    L.kmax = max(L.kmax, (unsigned)__shfl_xor((int)L.kmax, off));
  }
  constexpr int W = kMsThreads / 64;
  __shared__ unsigned r_nan[W], r_min[W], r_max[W];
  __shared__ long long r_sum[W];
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    r_nan[w] = L.nan; r_sum[w] = L.sum; r_min[w] = L.kmin; r_max[w] = L.kmax;
  }
  __syncthreads();                                          // (also: every lane's LDS histogram add is done)
  if (threadIdx.x == 0) {
    unsigned n = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
    long long s = 0;
    for (int w = 0; w < W; ++w) {
      n += r_nan[w]; s += r_sum[w]; kmin = min(kmin, r_min[w]); kmax = max(kmax, r_max[w]);
    }
    if (n) atomicAdd(rec + 0, (unsigned long long)n);
    if (s) atomicAdd(rec + 1, (unsigned long long)s);       // (two's complement: the slot is read back as a signed sum)
    if (kmin <= kmax) {                                     // at least one number was seen
      atomicMin(rec + 2, (unsigned long long)kmin);
      atomicMax(rec + 3, (unsigned long long)kmax);
    }
  }
  for (int i = threadIdx.x; i < bins + 2; i += kMsThreads) {
    const unsigned h = hist[i];
    if (h) atomicAdd(rec + 4 + i, (unsigned long long)h);
  }
}

// workgroup = (o * T + t) * tiles + tile
__global__ __launch_bounds__(kMsThreads) void membrane_stats_run_kernel(const float* __restrict__ v, int64_t run, int T, int tiles, MsBins B,
                                                                        unsigned long long* __restrict__ table) {
  __shared__ unsigned hist[kMsMaxBins + 2];
  ms_hist_clear(hist, B.bins);
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t ot = blockIdx.x / (unsigned)tiles;
  const float* base = v + ot * run;
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) >> 2);   // floats in front of the first 16-byte boundary
  if (head > run) head = run;
  const int64_t nvec = (run - head) >> 2;
  const int64_t tail0 = head + (nvec << 2);                                                // first float behind the last whole vector
  const float4* body = reinterpret_cast<const float4*>(base + head);
  const int64_t v0 = (int64_t)tile * kMsTileVecs + threadIdx.x;
  // all of a lane's loads are issued before the first use (a vector behind the run's end is not loaded and not counted)
  float4 w[kMsVecs];
#pragma unroll
  for (int k = 0; k < kMsVecs; ++k) {
    const int64_t i = v0 + k * kMsThreads;
    w[k] = i < nvec ? body[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  MsLane L;
#pragma unroll
  for (int k = 0; k < kMsVecs; ++k) {
    if (v0 + k * kMsThreads < nvec) {
      ms_take(L, hist, B, w[k].x);
      ms_take(L, hist, B, w[k].y);
      ms_take(L, hist, B, w[k].z);
      ms_take(L, hist, B, w[k].w);
    }
  }
  if (tile == 0) {                                          // lanes 0 .. 2: the head floats, lanes 16 .. 18: the tail floats
    const int64_t i = threadIdx.x;
    if (i < head)
      ms_take(L, hist, B, base[i]);
    else if (i >= 16 && i < 19 && tail0 + (i - 16) < run)
      ms_take(L, hist, B, base[tail0 + (i - 16)]);
  }
  ms_workgroup_flush(L, hist, B.bins, table + (ot % T) * (4 + B.bins + 2));
}

__global__ __launch_bounds__(kMsThreads) void membrane_stats_rows_kernel(const float* __restrict__ v, int64_t rows, int C, int64_t row_stride,
                                                                         int T, int tiles, MsBins B, unsigned long long* __restrict__ table) {
  __shared__ unsigned hist[kMsMaxBins + 2];
  ms_hist_clear(hist, B.bins);
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t ot = blockIdx.x / (unsigned)tiles;
  const float* base = v + ot * rows * row_stride;
  const int64_t n = rows * C, i0 = (int64_t)tile * kMsTileElems + threadIdx.x;
  MsLane L;
#pragma unroll 4
  for (int k = 0; k < kMsElems; ++k) {
    const int64_t i = i0 + k * kMsThreads;
    if (i < n) {
      const int64_t r = i / C;
      ms_take(L, hist, B, base[r * row_stride + (i - r * C)]);
    }
  }
  ms_workgroup_flush(L, hist, B.bins, table + (ot % T) * (4 + B.bins + 2));
}

}  // namespace

extern "C" int sdf_membrane_stats_fwd(const SdfMembraneStatsDesc* d, void* stream) {
  if (!d || !d->v || !d->table) return SDF_E_NULL;
  if (d->outer < 1 || d->rows < 1 || d->C < 1 || d->T < 1 || d->T > 64 || d->row_stride < d->C) return SDF_E_SHAPE;
  if (d->bins < 1 || d->bins > kMsMaxBins || !(d->lo < d->hi) || !(d->inv_width > 0.f) || !(d->inv_width < __builtin_inff())) return SDF_E_SHAPE;
  if (!sdf_aligned(d->v, 4) || !sdf_aligned(d->table, 8)) return SDF_E_ALIGN;
  // the last float's offset stays inside 60 bits (62 in bytes) and the grid inside 31
  const int64_t blocks = d->outer * d->T;
  if (d->outer > (1ll << 31) / d->T || d->rows > ((1ll << 60) / d->row_stride) / blocks) return SDF_E_SHAPE;
  const bool dense = d->row_stride == d->C;
  const int64_t per = dense ? (d->rows * d->C) >> 2 : d->rows * d->C, tile = dense ? kMsTileVecs : kMsTileElems;
  const int64_t tiles = per / tile + (per % tile != 0 || per == 0);
  if (tiles >= (1ll << 31) / blocks) return SDF_E_SHAPE;
  hipStream_t s = sdf_stream(stream);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(d->table);
  MsBins B;
  B.bins = d->bins; B.lo = d->lo; B.hi = d->hi; B.inv_width = d->inv_width;
  if (dense)
    SDF_LAUNCH(membrane_stats_run_kernel, dim3((unsigned)(blocks * tiles)), dim3(kMsThreads), 0, s, d->v, d->rows * d->C, d->T, (int)tiles, B,
               table);
  else
    SDF_LAUNCH(membrane_stats_rows_kernel, dim3((unsigned)(blocks * tiles)), dim3(kMsThreads), 0, s, d->v, d->rows, d->C, d->row_stride, d->T,
               (int)tiles, B, table);
  SDF_LAUNCH_CHECK();
  return 0;
}
