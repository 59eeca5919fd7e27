// Raw event lists -> voxel grid (the front end of "events in, flow out"), gfx950.
//
// Replaces the reference's VoxelGrid.convert_CHW / convert_CHW_polarities (DSEC_dataloader/event_representations.py:241-313: eight
// put_(accumulate=True) passes over the event list) and, fused behind it, what the evaluation loop does to the grid before the model
// sees it (eval_DSEC_flow_SNN.py:179-217: centre crop, polarity split, min-max over the non-zeros, spike threshold).
//
// No float atomics.  A cell's sum is formed by ONE lane in the order the reference's CPU put_ forms it: the eight corner passes in
// their order (x outer, y middle, t inner), events in list order inside a pass.  The order is made available by a stable sort of the
// events by the integer key of their BASE cell (x0, y0, t0): the run of base cell (X - dx, Y - dy, c - dt) in the sorted list is
// exactly the events pass (dx, dy, dt) adds to cell (c, Y, X), in list order.  The sort itself is the caller's (sdf_event_voxel_keys_fwd
// writes the keys, the caller sorts them stably, sdf_event_voxel_gather_fwd takes the sorted keys and the permutation); nothing here
// depends on how the events are split over workgroups, so two runs - or two different batchings - give the same bits.
//
// Launch sequence: keys (one launch per list) | [caller: stable sort] | clear the run table | runs + permute | [clear the min / max
// pair] | gather (+ min / max) | [finish: min-max, threshold].
#include "event_common.h"
#include "model_input.h"

namespace {

struct EvGeom {
  int32_t B, C, h, w, ox, oy;    // output window (h, w) at offset (oy, ox) inside the (H, W) sensor grid
  int32_t KT;                    // number of keys = B (C + 1) (h + 1) (w + 1); KT itself = "touches no output cell"
};

__device__ __forceinline__ int ev_key(const EvGeom& g, int b, int kt, int ky, int kx) {
  return ((b * (g.C + 1) + kt) * (g.h + 1) + ky) * (g.w + 1) + kx;
}

// XY: the coordinates' form (event_common.h event_load_xy)
template <int XY>
__global__ __launch_bounds__(256) void ev_keys_kernel(const void* __restrict__ xs, const void* __restrict__ ys, const float* __restrict__ t,
                                                      const float* __restrict__ p, const float* __restrict__ map, int map_h, int map_w,
                                                      int64_t i0, int n, int b, EvGeom g, int* __restrict__ keys, float4* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e = i0 + i;
  float x, y;
  bool ok = event_load_xy<XY>(xs, ys, map, map_h, map_w, e, x, y);
  // t_norm = (C - 1) (t - t[0]) / (t[N-1] - t[0]): multiply, then divide, each rounded to fp32 (event_representations.py:255)
  const float t_first = t[i0], t_last = t[i0 + n - 1];
  const float tn = ((float)(g.C - 1) * (t[e] - t_first)) / (t_last - t_first);
  // float range first (NaN fails every comparison), so that the truncations below are exact
  ok = ok && x > (float)(g.ox - 2) && x < (float)(g.ox + g.w + 1) && y > (float)(g.oy - 2) && y < (float)(g.oy + g.h + 1) &&
       tn > -2.f && tn < (float)(g.C + 1);
  int key = g.KT;
  if (ok) {
    const int kx = (int)x - g.ox + 1, ky = (int)y - g.oy + 1, kt = (int)tn + 1;      // .int(): truncation toward zero
    if (kx >= 0 && kx <= g.w && ky >= 0 && ky <= g.h && kt >= 0 && kt <= g.C) key = ev_key(g, b, kt, ky, kx);
  }
  keys[e] = key;
  rec[e] = make_float4(x, y, tn, p[e]);
}

// weight of an event for the corner at (xc, yc, tc): three fp32 products in the reference's order, nothing contracted
template <int MODE>
__device__ __forceinline__ void ev_add(const float4 r, float xc, float yc, float tc, float& acc, float& acc2) {
  const float wx = 1.f - fabsf(xc - r.x), wy = 1.f - fabsf(yc - r.y), wt = 1.f - fabsf(tc - r.z);
  if (MODE == 2) {
    const float wgt = (wx * wy) * wt;
    if (r.w == 1.f) acc += wgt;
    if (r.w == 0.f) acc2 += wgt;
  } else {
    acc += (((2.f * r.w - 1.f) * wx) * wy) * wt;
  }
}

// ev_add as the lane of cell (xc, yc, tc) applies it (event_common.h event_sum_run)
template <int MODE>
struct EvTerm {
  float xc, yc, tc;
  __device__ __forceinline__ void operator()(const float4 r, float& acc, float& acc2) const { ev_add<MODE>(r, xc, yc, tc, acc, acc2); }
  __device__ __forceinline__ EvTerm of_lane(int L) const { return EvTerm{__shfl(xc, L), __shfl(yc, L), __shfl(tc, L)}; }
};

// MODE 0: signed grid (B, C, h, w).  1: relu(v) | relu(-v) as (B, C, 2, h, w) (+ min / max of the non-zeros into mm when asked).
// 2: convert_CHW_polarities, unsigned weights of the p == 1 | p == 0 events as (B, C, 2, h, w).
template <int MODE>
__global__ __launch_bounds__(256) void ev_gather_kernel(const int2* __restrict__ tab, const float4* __restrict__ rec, float* __restrict__ out,
                                                        unsigned* __restrict__ mm, EvGeom g, int want_minmax) {
  const int64_t total = (int64_t)g.B * g.C * g.h * g.w;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool active = idx < total;
  const int64_t cell = active ? idx : 0;
  const int lane = threadIdx.x & 63;
  const int xx = (int)(cell % g.w), yy = (int)((cell / g.w) % g.h);
  const int c = (int)((cell / ((int64_t)g.w * g.h)) % g.C), b = (int)(cell / ((int64_t)g.w * g.h * g.C));
  const float xc = (float)(xx + g.ox), yc = (float)(yy + g.oy), tc = (float)c;
  float acc = 0.f, acc2 = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 8; ++pass) {
    const int dx = pass >> 2, dy = (pass >> 1) & 1, dt = pass & 1;      // x outer, y middle, t inner
    int2 r = make_int2(0, 0);
    if (active) r = tab[ev_key(g, b, c - dt + 1, yy - dy + 1, xx - dx + 1)];
    event_sum_run<MODE == 2>(r, rec, lane, EvTerm<MODE>{xc, yc, tc}, acc, acc2);
  }
  const int64_t hw = (int64_t)g.h * g.w, plane = (int64_t)yy * g.w + xx, bc = (int64_t)b * g.C + c;
  if (MODE == 0) {
    if (active) out[idx] = acc;
    return;
  }
  float* pair = out + (bc * 2) * hw + plane;
  if (MODE == 2) {
    if (active) {
      pair[0] = acc;
      pair[hw] = acc2;
    }
    return;
  }
  unsigned nlo = 0u, hi = 0u;                                            // (~min, max) over nothing
  if (active) mi_split_store(acc, pair, hw, nlo, hi);
  if (want_minmax) mi_minmax_commit_wave(nlo, hi, mm);                   // (no LDS or barrier in this kernel: a pair per wave)
}

// harness.prepare_chunk's tail on output 1, in place (model_input.h mi_finish_value), as a grid-stride pass over the elements: there is
// no event mask to form here, so the pass needs no lane per pixel (prepare_finish_kernel's shape: profiles/data_path_shared_code.txt)
__global__ __launch_bounds__(256) void ev_finish_kernel(float* __restrict__ out, int64_t n, const unsigned* __restrict__ mm, int want_minmax,
                                                        int want_th, float th) {
  float lo, span;
  const bool norm = mi_norm_of(mm, want_minmax, lo, span);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = out[i];
    mi_finish_value(v, norm, lo, span, want_th, th);
    out[i] = v;
  }
}

struct EvPlan {
  EvGeom g;
  int64_t off_rec, off_rec_s, off_tab, off_mm, bytes;
};

// geometry and workspace layout; false = SDF_E_SHAPE
bool ev_plan(int64_t n, int B, int C, int H, int W, int crop_h, int crop_w, EvPlan& pl) {
  if (n < 0 || n >= (1ll << 31) - 64 || B < 1 || C < 1 || H < 1 || W < 1 || crop_h < 0 || crop_w < 0 || crop_h > H || crop_w > W) return false;
  if ((crop_h == 0) != (crop_w == 0)) return false;
  EvGeom& g = pl.g;
  g.B = B;
  g.C = C;
  g.h = crop_h ? crop_h : H;
  g.w = crop_w ? crop_w : W;
  g.oy = (H - g.h) / 2;            // harness.center_crop
  g.ox = (W - g.w) / 2;
  const int64_t KT = (int64_t)B * (C + 1) * (g.h + 1) * (g.w + 1);
  if (KT >= (1ll << 31) - 1 || (int64_t)B * C * 2 * g.h * g.w >= (1ll << 40)) return false;
  g.KT = (int)KT;
  pl.off_rec = 0;
  pl.off_rec_s = pl.off_rec + pad256(n * 16);
  pl.off_tab = pl.off_rec_s + pad256(n * 16);
  pl.off_mm = pl.off_tab + pad256(KT * 8);
  pl.bytes = pl.off_mm + 256;
  return true;
}

int ev_check(const SdfEventVoxelDesc* d, EvPlan& pl, const int64_t*& offs, int64_t* own) {
  if (!d) return SDF_E_NULL;
  if (!ev_plan(d->n_events, d->B, d->C, d->H, d->W, d->crop_h, d->crop_w, pl)) return SDF_E_SHAPE;
  if (d->mode < 0 || d->mode > 2 || d->norm < 0 || d->norm > 1 || d->xy_dtype < 0 || d->xy_dtype > 2) return SDF_E_DTYPE;
  if (d->mode != 1 && (d->norm || d->use_spike_th)) return SDF_E_DTYPE;          // normalisation and threshold belong to the model-input form
  if (!d->workspace || !d->out) return SDF_E_NULL;
  if (d->workspace_bytes < pl.bytes) return SDF_E_SHAPE;
  if (!sdf_aligned(d->workspace, 16) || !sdf_aligned(d->out, 4)) return SDF_E_ALIGN;
  return event_lists_check(d->offsets, d->B, d->n_events, d->t_range, offs, own);
}

}  // namespace

extern "C" int64_t sdf_event_voxel_workspace_bytes(int64_t n_events, int B, int C, int H, int W, int crop_h, int crop_w) {
  EvPlan pl;
  return ev_plan(n_events, B, C, H, W, crop_h, crop_w, pl) ? pl.bytes : 0;
}

extern "C" int sdf_event_voxel_keys_fwd(const SdfEventVoxelDesc* d, void* stream) {
  EvPlan pl;
  const int64_t* offs;
  int64_t own[2];
  if (int rc = ev_check(d, pl, offs, own)) return rc;
  if (d->n_events == 0) return 0;
  if (int rc = event_keys_check(d->x, d->y, d->t, d->p, d->keys, d->xy_dtype, 4, true, d->rectify_map, d->map_h, d->map_w)) return rc;
  hipStream_t s = sdf_stream(stream);
  float4* rec = reinterpret_cast<float4*>(static_cast<char*>(d->workspace) + pl.off_rec);
  return event_keys_launch(offs, d->B, d->xy_dtype, [&](auto xy, dim3 grid, int64_t i0, int n, int b) {
    SDF_LAUNCH(ev_keys_kernel<decltype(xy)::value>, grid, dim3(256), 0, s, d->x, d->y, d->t, d->p, d->rectify_map, d->map_h, d->map_w, i0, n,
               b, pl.g, d->keys, rec);
  });
}

extern "C" int sdf_event_voxel_gather_fwd(const SdfEventVoxelDesc* d, void* stream) {
  EvPlan pl;
  const int64_t* offs;
  int64_t own[2];
  if (int rc = ev_check(d, pl, offs, own)) return rc;
  const int n = (int)d->n_events;
  hipStream_t s = sdf_stream(stream);
  char* ws = static_cast<char*>(d->workspace);
  const float4* rec = reinterpret_cast<const float4*>(ws + pl.off_rec);
  float4* rec_s = reinterpret_cast<float4*>(ws + pl.off_rec_s);
  int2* tab = reinterpret_cast<int2*>(ws + pl.off_tab);
  unsigned* mm = reinterpret_cast<unsigned*>(ws + pl.off_mm);
  const EvGeom& g = pl.g;
  if (int rc = event_runs_launch(d->keys_sorted, d->order, rec, rec_s, tab, n, g.KT, s)) return rc;
  if (d->norm)
    if (int rc = mi_clear_pairs(mm, 1, s)) return rc;
  const int64_t cells = (int64_t)g.B * g.C * g.h * g.w;
  const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
  float* out = static_cast<float*>(d->out);
  if (d->mode == 0) SDF_LAUNCH(ev_gather_kernel<0>, grid, block, 0, s, tab, rec_s, out, mm, g, 0);
  else if (d->mode == 1) SDF_LAUNCH(ev_gather_kernel<1>, grid, block, 0, s, tab, rec_s, out, mm, g, d->norm);
  else SDF_LAUNCH(ev_gather_kernel<2>, grid, block, 0, s, tab, rec_s, out, mm, g, 0);
  SDF_LAUNCH_CHECK();
  if (d->mode == 1 && (d->norm || d->use_spike_th)) {
    const int64_t nout = cells * 2;
    const unsigned blocks = (unsigned)((nout + 255) / 256 < 2048 ? (nout + 255) / 256 : 2048);
    SDF_LAUNCH(ev_finish_kernel, dim3(blocks), block, 0, s, out, nout, mm, d->norm, d->use_spike_th, d->spike_th);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}
