// The skeleton the two event front ends share (event_voxel.hip, event_voxel_tb.hip), stated once: the run table of the stably
// sorted events, the ordered summation of one pass over a cell's run, the ReLU and min / max of the model-input form, and the
// launchers' checks and run-table preamble.  What differs stays in the files: the keys, the record (float4 | float2), one event's
// term (ev_add | tb_add) and the passes of a cell.
#pragma once
#include "common.h"

namespace {

constexpr int kLongRun = 48;     // runs at least this long are summed by their lane with the whole wave fetching and weighting for it

// sorted position i: the event's record moves to its sorted place, and the first / last position of a key's run go to the run table
template <typename Rec>
__global__ __launch_bounds__(256) void event_runs_kernel(const int* __restrict__ ks, const int64_t* __restrict__ order,
                                                         const Rec* __restrict__ rec, int n, int KT, Rec* __restrict__ rec_s,
                                                         int2* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = ks[i];
  if (k < 0 || k >= KT) return;
  const int64_t e = order[i];
  if (e < 0 || e >= n) return;
  rec_s[i] = rec[e];
  if (i == 0 || ks[i - 1] != k) tab[k].x = i;
  if (i == n - 1 || ks[i + 1] != k) tab[k].y = i + 1;
}

// One pass of a cell: the events of run r = [r.x, r.y) of the sorted records are added to this lane's acc (TWO: acc | acc2 by
// polarity) in list order - the order is what makes the result the reference's, bit for bit.  A short run is summed by its own lane.
// A run of at least kLongRun is fetched and weighted by the whole wave, 64 events at a time, and added by the owning lane L one event
// after the other.  `term(record, a, a2)` adds one event's term as this lane's cell weights it; `term.of_lane(L)` is the functor as
// lane L holds it (wave-uniform).  Every lane of the wave calls this, a lane without a cell with an empty run.
template <bool TWO, typename Rec, typename Term>
__device__ __forceinline__ void event_sum_run(const int2 r, const Rec* rec, const int lane, const Term term, float& acc_io,
                                              float& acc2_io) {
  float acc = acc_io, acc2 = acc2_io;            // (locals: through the references the owning lane's add became a branch per event)
  const bool is_long = r.y - r.x >= kLongRun;
  if (!is_long)
    for (int i = r.x; i < r.y; ++i) term(rec[i], acc, acc2);
  unsigned long long todo = __ballot(is_long);
  while (todo) {                                                         // (wave-uniform)
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int s = __shfl(r.x, L), e = __shfl(r.y, L);
    const Term lterm = term.of_lane(L);
    for (int base = s; base < e; base += 64) {
      float w1 = 0.f, w2 = 0.f;
      if (base + lane < e) lterm(rec[base + lane], w1, w2);              // 0 + w = w: lane j holds event j's term
      const int cnt = min(64, e - base);
      for (int j = 0; j < cnt; ++j) {
        const float a1 = __shfl(w1, j);
        // (adding a skipped event's + 0 - TWO: the other polarity's - leaves acc as it is: acc is never - 0)
        if (lane == L) acc += a1;
        if (TWO) {
          const float a2 = __shfl(w2, j);
          if (lane == L) acc2 += a2;
        }
      }
    }
  }
  acc_io = acc;
  acc2_io = acc2;
}

// relu as ATen's device clamp_min forms it: NaN stays, else fmaxf(v, 0) = v_max_f32, which orders -0 below +0: relu(-0) = +0
__device__ __forceinline__ float event_relu(float v) { return v != v ? v : fmaxf(v, 0.f); }

// min / max of the non-zero outputs.  They are positive floats here, which order as their bit patterns: integer min / max, any arrival
// order.  Start from lo = 0xffffffff, hi = 0 ("no non-zero element").  The atomics behind the wave's reduction stay in the files:
// event_voxel.hip's gather kernel issues a pair per wave (one value per lane, no LDS or barrier in that kernel), event_voxel_tb.hip's
// grid-stride pass a pair per workgroup through LDS (a pair per wave cost more than that pass itself).
__device__ __forceinline__ void minmax_nonzero(float o, unsigned& lo, unsigned& hi) {
  if (o != 0.f) {
    lo = min(lo, __float_as_uint(o));
    hi = max(hi, __float_as_uint(o));
  }
}
__device__ __forceinline__ void wave_minmax(unsigned& lo, unsigned& hi) {
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
  }
}

inline int64_t pad256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// `offs` cuts n events into `lists` lists: from 0 to n, never backwards
inline bool event_offsets_ok(const int64_t* offs, int lists, int64_t n) {
  if (offs[0] != 0 || offs[lists] != n) return false;
  for (int b = 0; b < lists; ++b)
    if (offs[b + 1] < offs[b]) return false;
  return true;
}

// The head of a gather launcher: the caller's sorted keys and permutation are there and aligned; every run empty; min / max over
// nothing when they are wanted; then the run table and the sorted records.  0 or the error.
template <typename Rec>
inline int event_runs_launch(const int32_t* keys_sorted, const int64_t* order, const Rec* rec, Rec* rec_s, int2* tab, unsigned* mm, int n,
                             int KT, int want_minmax, hipStream_t s) {
  if (n && (!keys_sorted || !order)) return SDF_E_NULL;
  if (n && (!sdf_aligned(keys_sorted, 4) || !sdf_aligned(order, 8))) return SDF_E_ALIGN;
  hipError_t e = hipMemsetAsync(tab, 0, (size_t)KT * 8, s);             // every run empty
  if (e != hipSuccess) return (int)e;
  if (want_minmax) {
    e = hipMemsetAsync(mm, 0xff, 4, s);                                  // min over nothing
    if (e == hipSuccess) e = hipMemsetAsync(mm + 1, 0, 4, s);            // max over nothing: "no non-zero element"
    if (e != hipSuccess) return (int)e;
  }
  if (n) {
    SDF_LAUNCH(event_runs_kernel<Rec>, dim3((n + 255) / 256), dim3(256), 0, s, keys_sorted, order, rec, n, KT, rec_s, tab);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
