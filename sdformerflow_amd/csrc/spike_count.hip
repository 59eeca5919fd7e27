// u8 spikes -> per-time-step spike counts (the numerator of a firing rate), gfx950.
//
// Replaces, per neuron call, the reference's `cal_firing_rate(s_seq) = s_seq.flatten(1).mean(1)` of its output monitor
// (eval_DSEC_flow_SNN.py:22-24, 140-143): counts[t] += sum over (o, r, c) of spikes[((o T + t) rows + r) row_stride + c].  The counts are
// 64-bit integers the call ADDS to, so a table of every call of every forward accumulates on the device and is read back once; integer
// addition is order-independent: the atomics below give the same bits on every run.
//
// Two kernels:
//   run   row_stride == C: every (o, t) is ONE run of rows * C bytes.  16 bytes per lane from the first 16-byte boundary inside the
//         run; the bytes in front of it and behind the last whole vector are read one by one by the run's first workgroup, so that
//         nothing outside [base, base + run) is touched whatever the base's alignment (the bytes around a workspace slice belong to
//         other layers).  Four bytes are added per v_sad_u8 (sum of |byte - 0| + accumulator).
//   rows  row_stride > C (channel slices, the halves of a stacked q | k buffer: small tensors): element i of an (o, t) block is byte
//         i % C of row i / C.
// Both: lane -> wave -> workgroup, then one 64-bit atomic add per workgroup into counts[t].
//
// sdf_spike_count_seg_fwd is the same count per SAMPLE: element (so, t, si, r, c) at ((((so T + t) s_in + si) rows + r) row_stride + c,
// counts[(so s_in + si) sample_pitch + t] += sum over r, c.  s_in = 1: samples outside time (channel-last (B, D, h, w, C) records);
// s_out = 1: the samples are s_in equal consecutive pieces of every time block (the "flat" records of a replica forward).  Every
// (so, t, si) piece is a run of its own - its head and tail bytes are read one by one, so no byte of a neighbouring piece (another
// sample) is read, let alone added.  The two reduction bodies are stated once (sc_run_body, sc_rows_body): the kernels differ in where
// a run starts and which counter it adds to.
#include "common.h"

namespace {

constexpr int kScThreads = 256;
constexpr int kScVecs = 8;                                  // 16-byte loads per lane
constexpr int kScTileVecs = kScThreads * kScVecs;           // per workgroup: 2 048 vectors = 32 KiB of a run
constexpr int kScElems = 32;                                // rows kernel: bytes per lane
constexpr int kScTileElems = kScThreads * kScElems;

// Overflow bound of the 32-bit accumulators: a lane adds at most kScVecs * 16 + 1 = 129 bytes (run kernel: its vectors and one head or
// tail byte) or kScElems = 32 bytes (rows kernel) of at most 255 each: < 2^16; the 256 lanes of a workgroup together < 2^24.  The sum
// is widened to 64 bits at the atomic.
__device__ __forceinline__ unsigned sc_add4(unsigned w, unsigned acc) { return __builtin_amdgcn_sad_u8(w, 0u, acc); }

__device__ __forceinline__ void sc_workgroup_add(unsigned v, unsigned long long* dst) {
  for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off);
  __shared__ unsigned red[kScThreads / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned s = (red[0] + red[1]) + (red[2] + red[3]);
    if (s) atomicAdd(dst, (unsigned long long)s);
  }
}

// The run body: workgroup `tile` of the run [base, base + run) adds its bytes to *dst.
__device__ __forceinline__ void sc_run_body(const uint8_t* __restrict__ base, int64_t run, int tile, unsigned long long* dst) {
  int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15);     // bytes in front of the first 16-byte boundary
  if (head > run) head = run;
  const int64_t nvec = (run - head) >> 4;
  const int64_t tail0 = head + (nvec << 4);                                            // first byte behind the last whole vector
  const uint4* body = reinterpret_cast<const uint4*>(base + head);
  const int64_t v0 = (int64_t)tile * kScTileVecs + threadIdx.x;
  // all of a lane's loads are issued before the first sum (a vector behind the run's end reads as zeros and is not loaded)
  uint4 w[kScVecs];
#pragma unroll
  for (int k = 0; k < kScVecs; ++k) {
    const int64_t v = v0 + k * kScThreads;
    w[k] = v < nvec ? body[v] : make_uint4(0u, 0u, 0u, 0u);
  }
  unsigned acc = 0;
#pragma unroll
  for (int k = 0; k < kScVecs; ++k) acc = sc_add4(w[k].w, sc_add4(w[k].z, sc_add4(w[k].y, sc_add4(w[k].x, acc))));
  if (tile == 0) {                                          // lanes 0 .. 14: the head bytes, lanes 16 .. 30: the tail bytes
    const int64_t i = threadIdx.x;
    if (i < head)
      acc += base[i];
    else if (i >= 16 && tail0 + (i - 16) < run)
      acc += base[tail0 + (i - 16)];
  }
  sc_workgroup_add(acc, dst);
}

// The rows body: workgroup `tile` of the rows x C block at `base` (rows row_stride apart) adds its bytes to *dst.
__device__ __forceinline__ void sc_rows_body(const uint8_t* __restrict__ base, int64_t rows, int C, int64_t row_stride, int tile,
                                             unsigned long long* dst) {
  const int64_t n = rows * C, i0 = (int64_t)tile * kScTileElems + threadIdx.x;
  unsigned acc = 0;
#pragma unroll 4
  for (int k = 0; k < kScElems; ++k) {
    const int64_t i = i0 + k * kScThreads;
    if (i < n) {
      const int64_t r = i / C;
      acc += base[r * row_stride + (i - r * C)];
    }
  }
  sc_workgroup_add(acc, dst);
}

// The counter of piece p = (so * T + t) * s_in + si of the per-sample kernels: sample so * s_in + si, step t.
__device__ __forceinline__ unsigned long long* sc_seg_counter(unsigned long long* counts, int64_t p, int T, int64_t s_in,
                                                              int64_t sample_pitch) {
  const int64_t ot = p / s_in, si = p - ot * s_in;
  const int64_t so = ot / T, t = ot - so * T;
  return counts + (so * s_in + si) * sample_pitch + t;
}

// workgroup = (o * T + t) * tiles + tile
__global__ __launch_bounds__(kScThreads) void spike_count_run_kernel(const uint8_t* __restrict__ spikes, int64_t run, int T, int tiles,
                                                                     unsigned long long* __restrict__ counts) {
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t ot = blockIdx.x / (unsigned)tiles;
  sc_run_body(spikes + ot * run, run, tile, counts + ot % T);
}

__global__ __launch_bounds__(kScThreads) void spike_count_rows_kernel(const uint8_t* __restrict__ spikes, int64_t rows, int C,
                                                                      int64_t row_stride, int T, int tiles,
                                                                      unsigned long long* __restrict__ counts) {
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t ot = blockIdx.x / (unsigned)tiles;
  sc_rows_body(spikes + ot * rows * row_stride, rows, C, row_stride, tile, counts + ot % T);
}

// workgroup = ((so * T + t) * s_in + si) * tiles + tile: every (so, t, si) piece is a run of its own
__global__ __launch_bounds__(kScThreads) void spike_count_seg_run_kernel(const uint8_t* __restrict__ spikes, int64_t run, int T,
                                                                         int64_t s_in, int tiles, int64_t sample_pitch,
                                                                         unsigned long long* __restrict__ counts) {
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t p = blockIdx.x / (unsigned)tiles;
  sc_run_body(spikes + p * run, run, tile, sc_seg_counter(counts, p, T, s_in, sample_pitch));
}

__global__ __launch_bounds__(kScThreads) void spike_count_seg_rows_kernel(const uint8_t* __restrict__ spikes, int64_t rows, int C,
                                                                          int64_t row_stride, int T, int64_t s_in, int tiles,
                                                                          int64_t sample_pitch, unsigned long long* __restrict__ counts) {
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const int64_t p = blockIdx.x / (unsigned)tiles;
  sc_rows_body(spikes + p * rows * row_stride, rows, C, row_stride, tile, sc_seg_counter(counts, p, T, s_in, sample_pitch));
}

// workgroups per run: whole 16-byte vectors (dense) or elements (strided) over a workgroup's tile, one at least
int64_t sc_tiles(bool dense, int64_t rows, int C) {
  const int64_t per = dense ? (rows * C) >> 4 : rows * C, tile = dense ? kScTileVecs : kScTileElems;
  return per / tile + (per % tile != 0 || per == 0);
}

}  // namespace

extern "C" int sdf_spike_count_fwd(const SdfSpikeCountDesc* d, void* stream) {
  if (!d || !d->spikes || !d->counts) return SDF_E_NULL;
  if (d->outer < 1 || d->rows < 1 || d->C < 1 || d->T < 1 || d->T > 64 || d->row_stride < d->C) return SDF_E_SHAPE;
  if (!sdf_aligned(d->counts, 8)) return SDF_E_ALIGN;
  // the last byte's offset stays inside 62 bits and the grid inside 31
  const int64_t blocks = d->outer * d->T;
  if (d->outer > (1ll << 31) / d->T || d->rows > ((1ll << 62) / d->row_stride) / blocks) return SDF_E_SHAPE;
  const bool dense = d->row_stride == d->C;
  const int64_t tiles = sc_tiles(dense, d->rows, d->C);
  if (tiles >= (1ll << 31) / blocks) return SDF_E_SHAPE;
  hipStream_t s = sdf_stream(stream);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(d->counts);
  if (dense)
    SDF_LAUNCH(spike_count_run_kernel, dim3((unsigned)(blocks * tiles)), dim3(kScThreads), 0, s, d->spikes, d->rows * d->C, d->T, (int)tiles,
               counts);
  else
    SDF_LAUNCH(spike_count_rows_kernel, dim3((unsigned)(blocks * tiles)), dim3(kScThreads), 0, s, d->spikes, d->rows, d->C, d->row_stride,
               d->T, (int)tiles, counts);
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_spike_count_seg_fwd(const SdfSpikeCountSegDesc* d, void* stream) {
  if (!d || !d->spikes || !d->counts) return SDF_E_NULL;
  if (d->s_out < 1 || d->s_in < 1 || d->rows < 1 || d->C < 1 || d->T < 1 || d->T > 64 || d->row_stride < d->C || d->sample_pitch < d->T)
    return SDF_E_SHAPE;
  if (!sdf_aligned(d->counts, 8)) return SDF_E_ALIGN;
  // the last byte's offset (of the spikes and of the counts) stays inside 62 bits and the grid inside 31
  if (d->s_out > (1ll << 31) / d->T || d->s_in > ((1ll << 31) / d->T) / d->s_out) return SDF_E_SHAPE;
  const int64_t samples = d->s_out * d->s_in, pieces = samples * d->T;
  if (d->rows > ((1ll << 62) / d->row_stride) / pieces || d->sample_pitch > (1ll << 59) / samples) return SDF_E_SHAPE;
  const bool dense = d->row_stride == d->C;
  const int64_t tiles = sc_tiles(dense, d->rows, d->C);
  if (tiles >= (1ll << 31) / pieces) return SDF_E_SHAPE;
  hipStream_t s = sdf_stream(stream);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(d->counts);
  if (dense)
    SDF_LAUNCH(spike_count_seg_run_kernel, dim3((unsigned)(pieces * tiles)), dim3(kScThreads), 0, s, d->spikes, d->rows * d->C, d->T,
               d->s_in, (int)tiles, d->sample_pitch, counts);
  else
    SDF_LAUNCH(spike_count_seg_rows_kernel, dim3((unsigned)(pieces * tiles)), dim3(kScThreads), 0, s, d->spikes, d->rows, d->C,
               d->row_stride, d->T, d->s_in, (int)tiles, d->sample_pitch, counts);
  SDF_LAUNCH_CHECK();
  return 0;
}
