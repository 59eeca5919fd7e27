// The skeleton the three event front ends share (event_voxel.hip, event_voxel_tb.hip, event_iwe.hip), stated once: the coordinate
// load through the rectify map, the checks of the lists and of the keys call's inputs, the per-list keys launch with its coordinate
// dtype dispatch, the run table of the stably sorted events (with or without moving a record), and the ordered summation of one pass
// over a cell's run.  What differs stays in the files: the keys, the record (float4 | float2 | none), one event's term (ev_add | tb_add
// | IweTerm) and the passes of a cell.  event_voxel_tb.hip truncates integer pixels and has no map: its coordinate load is its own.
// The model-input tail behind the two voxel front ends is model_input.h's.
//
// An inconsistency that stays: the IWE calls refuse host memory (SDF_E_DTYPE, after NULL and alignment); event_voxel and event_voxel_tb
// make no device-memory check.
#pragma once
#include "common.h"
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int kLongRun = 48;     // runs at least this long are summed by their lane with the whole wave fetching and weighting for it

struct EventNoRec {};            // the record-free form: a cell's value is the length of its run (event_iwe.hip, nearest mode)

// XY: 0 = fp32 coordinates as given, 1 = int32 sensor coordinates through the rectify map (x, y <- map[y, x]), 2 = uint16 likewise.
// false: outside the map (the reference asserts this; here such an event adds nothing), x, y then the map's first entry
template <int XY>
__device__ __forceinline__ bool event_load_xy(const void* __restrict__ xs, const void* __restrict__ ys, const float* __restrict__ map,
                                              int map_h, int map_w, int64_t e, float& x, float& y) {
  if (XY == 0) {
    x = static_cast<const float*>(xs)[e];
    y = static_cast<const float*>(ys)[e];
    return true;
  }
  int xi, yi;
  if (XY == 1) {
    xi = static_cast<const int32_t*>(xs)[e];
    yi = static_cast<const int32_t*>(ys)[e];
  } else {
    xi = static_cast<const uint16_t*>(xs)[e];
    yi = static_cast<const uint16_t*>(ys)[e];
  }
  const bool ok = xi >= 0 && xi < map_w && yi >= 0 && yi < map_h;
  const int64_t m = ok ? ((int64_t)yi * map_w + xi) * 2 : 0;
  x = map[m];
  y = map[m + 1];
  return ok;
}

// sorted position i: the event's record moves to its sorted place (Rec = EventNoRec: there is none, `order` is not read), and the
// first / last position of a key's run go to the run table
template <typename Rec>
__global__ __launch_bounds__(256) void event_runs_kernel(const int* __restrict__ ks, const int64_t* __restrict__ order,
                                                         const Rec* __restrict__ rec, int n, int KT, Rec* __restrict__ rec_s,
                                                         int2* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = ks[i];
  if (k < 0 || k >= KT) return;
  if constexpr (!std::is_same<Rec, EventNoRec>::value) {
    const int64_t e = order[i];
    if (e < 0 || e >= n) return;
    rec_s[i] = rec[e];
  }
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

inline int64_t pad256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// `offs` cuts n events into `lists` lists: from 0 to n, never backwards
inline bool event_offsets_ok(const int64_t* offs, int lists, int64_t n) {
  if (offs[0] != 0 || offs[lists] != n) return false;
  for (int b = 0; b < lists; ++b)
    if (offs[b + 1] < offs[b]) return false;
  return true;
}

// `offsets` (NULL: the one list of a B = 1 call, written to `own`) and, when given, the lists' {first, last} times: 0 and `offs`, or
// the error
inline int event_lists_check(const int64_t* offsets, int B, int64_t n, const float* t_range, const int64_t*& offs, int64_t* own) {
  offs = offsets;
  if (!offs) {
    if (B != 1) return SDF_E_NULL;
    own[0] = 0;
    own[1] = n;
    offs = own;
  }
  if (!event_offsets_ok(offs, B, n)) return SDF_E_SHAPE;
  if (t_range)
    for (int b = 0; b < B; ++b)                                          // a list whose first and last time are equal has no t_norm
      if (offs[b + 1] > offs[b] && !(t_range[2 * b + 1] != t_range[2 * b])) return SDF_E_SHAPE;
  return 0;
}

// the inputs of a keys call with events: there | the rectify map (`mapped` entry points: required with integer coordinates, refused
// with fp32 ones, which do not index it) | aligned, t to `t_align` (4: fp32, 8: fp64)
inline int event_keys_check(const void* x, const void* y, const void* t, const void* p, const void* keys, int xy_dtype, size_t t_align,
                            bool mapped, const float* map, int map_h, int map_w) {
  if (!x || !y || !t || !p || !keys) return SDF_E_NULL;
  if (mapped && xy_dtype != 0 && (!map || map_h < 1 || map_w < 1)) return map ? SDF_E_SHAPE : SDF_E_NULL;
  if (mapped && xy_dtype == 0 && map) return SDF_E_DTYPE;
  const size_t xy_align = xy_dtype == 2 ? 2 : 4;
  if (!sdf_aligned(x, xy_align) || !sdf_aligned(y, xy_align) || !sdf_aligned(t, t_align) || !sdf_aligned(p, 4) || !sdf_aligned(keys, 4) ||
      (mapped && map && !sdf_aligned(map, 4)))
    return SDF_E_ALIGN;
  return 0;
}

template <int XY>
using EventXY = std::integral_constant<int, XY>;

// one keys launch per non-empty list: launch(EventXY<xy_dtype>, grid, first event, events, list) with 256 threads per workgroup
template <typename Launch>
inline int event_keys_launch(const int64_t* offs, int lists, int xy_dtype, Launch launch) {
  for (int b = 0; b < lists; ++b) {
    const int64_t i0 = offs[b];
    const int n = (int)(offs[b + 1] - i0);
    if (n == 0) continue;
    const dim3 grid((n + 255) / 256);
    if (xy_dtype == 0) launch(EventXY<0>{}, grid, i0, n, b);
    else if (xy_dtype == 1) launch(EventXY<1>{}, grid, i0, n, b);
    else launch(EventXY<2>{}, grid, i0, n, b);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}

// The head of a gather launcher: the caller's sorted keys and permutation are there and aligned - and, for an entry point that refuses
// host memory, on the device together with its other buffers `device` -; every run empty; then the run table and the sorted records
// (Rec = EventNoRec: the run table alone).  0 or the error.
template <typename Rec>
inline int event_runs_launch(const int32_t* keys_sorted, const int64_t* order, const Rec* rec, Rec* rec_s, int2* tab, int n, int KT,
                             hipStream_t s, std::initializer_list<const void*> device = {}) {
  if (n && (!keys_sorted || !order)) return SDF_E_NULL;
  if (n && (!sdf_aligned(keys_sorted, 4) || !sdf_aligned(order, 8))) return SDF_E_ALIGN;
  for (const void* p : device)
    if (!sdf_on_device(p)) return SDF_E_DTYPE;
  if (device.size() && n && (!sdf_on_device(keys_sorted) || !sdf_on_device(order))) return SDF_E_DTYPE;
  const hipError_t e = hipMemsetAsync(tab, 0, (size_t)KT * 8, s);       // every run empty
  if (e != hipSuccess) return (int)e;
  if (n) {
    SDF_LAUNCH(event_runs_kernel<Rec>, dim3((n + 255) / 256), dim3(256), 0, s, keys_sorted, order, rec, n, KT, rec_s, tab);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
