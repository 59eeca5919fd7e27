// Raw event lists + an estimated flow -> the image of warped events (IWE) and its statistics: flow quality without ground truth, gfx950.
//
// There is no reference implementation (the reference's Visualization_DSEC carries `iwe` slots its loops fill with None); this header and
// DESIGN.md section 5 are the specification, tests/iwe_cases.py restates it in numpy.
//
// Inputs: B event lists x, y, t, p back to back (x, y fp32 - or int32 / uint16 sensor coordinates through a rectify map; t fp32 in list
// order; p fp32), a flow (B, 2, h, w) fp32 (channel 0 = x) on the output window (h, w) at (oy, ox) of the (H, W) sensor, `scale`
// (multiplies the flow), `t_ref`, `window` (a, b), mode bilinear | nearest.  Per event, in fp32, every operation rounded on its own
// (the build does not contract):
//   1. tn = (t - t_first) / (t_last - t_first) of its list; skipped unless a <= tn <= b (a NaN fails); tau = (tn - a) / (b - a).
//   2. lookup pixel xi = (int)floorf(x + 0.5f) - ox, yi likewise (float range checked first); outside [0, w) x [0, h): skipped.
//   3. u = scale * flow[b, 0, yi, xi], v = scale * flow[b, 1, yi, xi]; skipped if either is not finite.
//   4. d = t_ref - tau;  xw = (x - ox) + d * u;  yw = (y - oy) + d * v.
//   5. channel 0 if p > 0, else channel 1.
//   6. bilinear: x0 = floorf(xw), y0 = floorf(yw); the corners (x0 + dx, y0 + dy) get (1 - |xc - xw|) * (1 - |yc - yw|); corners outside
//      the window are dropped.  A cell's sum is formed in the order: passes dx outer, dy inner, events in list order within a pass.
//      nearest: weight 1 at (rintf(xw), rintf(yw)), halves to even (-0 counts as 0), dropped if outside: the image holds integers.
// Output (B, 2, h, w) fp32; an empty list gives zeros.
//
// No float atomics.  As in event_voxel.hip a cell's sum is formed by ONE lane, the order made available by the caller's stable sort of the
// events by the integer key of their base cell - here (list, channel, y0, x0), so a lane owns one output ELEMENT and reads 8-byte records
// (xw, yw).  In nearest mode the base cell is the cell itself and its value is the length of its run: no record is stored or moved.
// Nothing depends on how the events are split over workgroups or lists over a batch: two runs, or two batchings, give the same bits.
//
// Launch sequence: keys (one launch per list) | [caller: stable sort] | clear the run table | event_runs_kernel (bilinear: + permute;
// nearest: its record-free form) | gather.
//
// sdf_iwe_stats_fwd: per sample {sum c, sum c^2, max c, pixels with c != 0} of c = the fp64 sum of a pixel's two channels, in
// record_table.h's form: lane -> wave -> workgroup -> one fp64 partial record per workgroup, then combined in index order.
// The Flow Warp Loss (Stoffregen et al. 2020) of a sample is var(S) / var(Z) on nearest images, S warped by the flow and Z by none, with
// var = (sum c^2 - (sum c)^2 / N) / (N - 1) in fp64 over the N = h w pixels: the sums are integers, exact while below 2^53.
#include "event_common.h"
#include "record_table.h"

namespace {

struct IweGeom {
  int32_t B, h, w, ox, oy;
  int32_t KT;                    // number of keys = B 2 (h + 1) (w + 1); KT itself = "touches no output cell"
};

// base cell (kx - 1, ky - 1) of channel c in list b
__device__ __forceinline__ int iwe_key(const IweGeom& g, int b, int c, int ky, int kx) {
  return ((b * 2 + c) * (g.h + 1) + ky) * (g.w + 1) + kx;
}

struct IweParams {
  float scale, t_ref, a, b;
};

// XY: the coordinates' form (event_common.h event_load_xy).  NEAREST: no record.
template <int XY, bool NEAREST>
__global__ __launch_bounds__(256) void iwe_keys_kernel(const void* __restrict__ xs, const void* __restrict__ ys, const float* __restrict__ t,
                                                       const float* __restrict__ p, const float* __restrict__ flow,
                                                       const float* __restrict__ map, int map_h, int map_w, int64_t i0, int n, int b,
                                                       IweGeom g, IweParams q, int* __restrict__ keys, float2* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e = i0 + i;
  float x, y;
  bool ok = event_load_xy<XY>(xs, ys, map, map_h, map_w, e, x, y);
  const float t_first = t[i0], t_last = t[i0 + n - 1];
  const float tn = (t[e] - t_first) / (t_last - t_first);
  ok = ok && tn >= q.a && tn <= q.b;                             // (NaN fails)
  const float tau = (tn - q.a) / (q.b - q.a);
  // lookup pixel: float range first (NaN fails every comparison), so that the conversions are exact
  const float fx = floorf(x + 0.5f), fy = floorf(y + 0.5f);
  ok = ok && fx >= (float)g.ox && fx < (float)(g.ox + g.w) && fy >= (float)g.oy && fy < (float)(g.oy + g.h);
  float xw = 0.f, yw = 0.f;
  int key = g.KT;
  if (ok) {
    const int xi = (int)fx - g.ox, yi = (int)fy - g.oy;
    const int64_t hw = (int64_t)g.h * g.w, at = (int64_t)b * 2 * hw + (int64_t)yi * g.w + xi;
    const float u = q.scale * flow[at], v = q.scale * flow[at + hw];
    const float d = q.t_ref - tau;
    xw = (x - (float)g.ox) + d * u;
    yw = (y - (float)g.oy) + d * v;
    const float bx = NEAREST ? rintf(xw) : floorf(xw), by = NEAREST ? rintf(yw) : floorf(yw);
    const float lo = NEAREST ? 0.f : -1.f;                       // (-0 >= 0: row / column 0)
    if (isfinite(u) && isfinite(v) && bx >= lo && bx < (float)g.w && by >= lo && by < (float)g.h)
      key = iwe_key(g, b, p[e] > 0.f ? 0 : 1, (int)by + 1, (int)bx + 1);
  }
  keys[e] = key;
  if (!NEAREST) rec[e] = make_float2(xw, yw);
}

// an event's weight at the corner (xc, yc), as the lane of that cell applies it (event_common.h event_sum_run)
struct IweTerm {
  float xc, yc;
  __device__ __forceinline__ void operator()(const float2 r, float& acc, float&) const {
    acc += (1.f - fabsf(xc - r.x)) * (1.f - fabsf(yc - r.y));
  }
  __device__ __forceinline__ IweTerm of_lane(int L) const { return IweTerm{__shfl(xc, L), __shfl(yc, L)}; }
};

// one lane per output element (b, channel, y, x)
template <bool NEAREST>
__global__ __launch_bounds__(256) void iwe_gather_kernel(const int2* __restrict__ tab, const float2* __restrict__ rec,
                                                         float* __restrict__ out, IweGeom g) {
  const int64_t total = (int64_t)g.B * 2 * g.h * g.w;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool active = idx < total;
  const int64_t cell = active ? idx : 0;
  const int xx = (int)(cell % g.w), yy = (int)((cell / g.w) % g.h);
  const int c = (int)((cell / ((int64_t)g.w * g.h)) % 2), b = (int)(cell / ((int64_t)g.w * g.h * 2));
  if (NEAREST) {
    if (active) {
      const int2 r = tab[iwe_key(g, b, c, yy + 1, xx + 1)];
      out[idx] = (float)(r.y - r.x);
    }
    return;
  }
  const int lane = threadIdx.x & 63;
  float acc = 0.f, unused = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 4; ++pass) {
    const int dx = pass >> 1, dy = pass & 1;                             // x outer, y inner
    int2 r = make_int2(0, 0);
    if (active) r = tab[iwe_key(g, b, c, yy - dy + 1, xx - dx + 1)];
    event_sum_run<false>(r, rec, lane, IweTerm{(float)xx, (float)yy}, acc, unused);
  }
  if (active) out[idx] = acc;
}

struct IwePlan {
  IweGeom g;
  int64_t off_rec, off_rec_s, off_tab, bytes;
};

// geometry and workspace layout; false = SDF_E_SHAPE.  mode 1 (nearest) keeps no records.
bool iwe_plan(int64_t n, int B, int H, int W, int crop_h, int crop_w, int crop_oy, int crop_ox, int mode, IwePlan& pl) {
  if (n < 0 || n >= (1ll << 31) - 64 || B < 1 || H < 1 || W < 1 || crop_h < 0 || crop_w < 0 || crop_h > H || crop_w > W) return false;
  if ((crop_h == 0) != (crop_w == 0)) return false;
  if (H >= (1 << 24) || W >= (1 << 24)) return false;                    // pixel numbers are exact in fp32
  IweGeom& g = pl.g;
  g.B = B;
  g.h = crop_h ? crop_h : H;
  g.w = crop_w ? crop_w : W;
  g.oy = crop_h ? crop_oy : 0;
  g.ox = crop_w ? crop_ox : 0;
  if (!crop_h && (crop_oy || crop_ox)) return false;
  if (g.oy < 0 || g.ox < 0 || g.oy + g.h > H || g.ox + g.w > W) return false;
  const int64_t KT = (int64_t)B * 2 * (g.h + 1) * (g.w + 1);
  if (KT >= (1ll << 31) - 1) return false;
  g.KT = (int)KT;
  const int64_t recs = mode == 1 ? 0 : pad256(n * 8);
  pl.off_rec = 0;
  pl.off_rec_s = pl.off_rec + recs;
  pl.off_tab = pl.off_rec_s + recs;
  pl.bytes = pl.off_tab + pad256(KT * 8);
  return true;
}

// the checks both calls share, in the family's order: NULL d | geometry | selectors | NULL buffers | workspace size | alignment | lists
int iwe_check(const SdfEventIweDesc* d, IwePlan& pl, const int64_t*& offs, int64_t* own) {
  if (!d) return SDF_E_NULL;
  if (!iwe_plan(d->n_events, d->B, d->H, d->W, d->crop_h, d->crop_w, d->crop_oy, d->crop_ox, d->mode, pl)) return SDF_E_SHAPE;
  if (d->mode < 0 || d->mode > 1 || d->xy_dtype < 0 || d->xy_dtype > 2) return SDF_E_DTYPE;
  if (!(d->win_a < d->win_b) || !isfinite(d->win_a) || !isfinite(d->win_b) || !isfinite(d->t_ref) || d->scale != d->scale) return SDF_E_SHAPE;
  if (!d->workspace || !d->out || !d->flow) return SDF_E_NULL;
  if (d->workspace_bytes < pl.bytes) return SDF_E_SHAPE;
  if (!sdf_aligned(d->workspace, 16) || !sdf_aligned(d->out, 4) || !sdf_aligned(d->flow, 4)) return SDF_E_ALIGN;
  return event_lists_check(d->offsets, d->B, d->n_events, d->t_range, offs, own);
}

constexpr int kIsFields = 4;
constexpr unsigned kIsMaxes = 1u << 2;                  // field 2 is a maximum

__global__ __launch_bounds__(kRtThreads) void iwe_stats_partial_kernel(const float* __restrict__ iwe, int hw, int nblk,
                                                                       double* __restrict__ part) {
  const int b = blockIdx.y;
  const float* c0 = iwe + (int64_t)b * 2 * hw;
  double s1 = 0.0, s2 = 0.0, mx = 0.0;
  unsigned nz = 0u;
#pragma unroll
  for (int k = 0; k < kRtPerLane; ++k) {
    const int i = blockIdx.x * kRtTile + k * kRtThreads + threadIdx.x;
    if (i >= hw) continue;
    const double c = (double)c0[i] + (double)c0[hw + i];
    s1 += c;
    s2 += c * c;
    mx = fmax(mx, c);
    nz += c != 0.0;
  }
  const double rec[kIsFields] = {rt_wave_sum(s1), rt_wave_sum(s2), rt_wave_max(mx), (double)rt_wave_sum(nz)};
  rt_block_store<kIsFields, kIsMaxes>(rec, part + ((int64_t)b * nblk + blockIdx.x) * kIsFields);
}

// sample blockIdx.x: lane k combines field k of the sample's partial records in index order
__global__ __launch_bounds__(64) void iwe_stats_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ rows) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= kIsFields) return;
  rows[(int64_t)b * kIsFields + k] = rt_finish_field<kIsFields, kIsMaxes>(part + (int64_t)b * nblk * kIsFields, nblk, k);
}

}  // namespace

extern "C" int64_t sdf_event_iwe_workspace_bytes(int64_t n_events, int B, int H, int W, int crop_h, int crop_w, int crop_oy, int crop_ox,
                                                 int mode) {
  IwePlan pl;
  if (mode < 0 || mode > 1) return 0;
  return iwe_plan(n_events, B, H, W, crop_h, crop_w, crop_oy, crop_ox, mode, pl) ? pl.bytes : 0;
}

extern "C" int sdf_event_iwe_keys_fwd(const SdfEventIweDesc* d, void* stream) {
  IwePlan pl;
  const int64_t* offs;
  int64_t own[2];
  if (int rc = iwe_check(d, pl, offs, own)) return rc;
  if (d->n_events == 0) return 0;
  if (int rc = event_keys_check(d->x, d->y, d->t, d->p, d->keys, d->xy_dtype, 4, true, d->rectify_map, d->map_h, d->map_w)) return rc;
  for (const void* ptr : {d->x, d->y, (const void*)d->t, (const void*)d->p, (const void*)d->flow, (const void*)d->keys,
                          (const void*)d->workspace})
    if (!sdf_on_device(ptr)) return SDF_E_DTYPE;
  if (d->rectify_map && !sdf_on_device(d->rectify_map)) return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  float2* rec = reinterpret_cast<float2*>(static_cast<char*>(d->workspace) + pl.off_rec);
  const IweParams q = {d->scale, d->t_ref, d->win_a, d->win_b};
  return event_keys_launch(offs, d->B, d->xy_dtype, [&](auto xy, dim3 grid, int64_t i0, int n, int b) {
    constexpr int XY = decltype(xy)::value;
    const auto kernel = d->mode == 0 ? iwe_keys_kernel<XY, false> : iwe_keys_kernel<XY, true>;
    SDF_LAUNCH(kernel, grid, dim3(256), 0, s, d->x, d->y, d->t, d->p, d->flow, d->rectify_map, d->map_h, d->map_w, i0, n, b, pl.g, q, d->keys,
               rec);
  });
}

extern "C" int sdf_event_iwe_gather_fwd(const SdfEventIweDesc* d, void* stream) {
  IwePlan pl;
  const int64_t* offs;
  int64_t own[2];
  if (int rc = iwe_check(d, pl, offs, own)) return rc;
  const int n = (int)d->n_events;
  hipStream_t s = sdf_stream(stream);
  char* ws = static_cast<char*>(d->workspace);
  const float2* rec = reinterpret_cast<const float2*>(ws + pl.off_rec);
  float2* rec_s = reinterpret_cast<float2*>(ws + pl.off_rec_s);
  int2* tab = reinterpret_cast<int2*>(ws + pl.off_tab);
  const IweGeom& g = pl.g;
  const int rc = d->mode == 0 ? event_runs_launch(d->keys_sorted, d->order, rec, rec_s, tab, n, g.KT, s, {d->out, d->workspace})
                              : event_runs_launch<EventNoRec>(d->keys_sorted, d->order, nullptr, nullptr, tab, n, g.KT, s,
                                                              {d->out, d->workspace});
  if (rc) return rc;
  const int64_t cells = (int64_t)g.B * 2 * g.h * g.w;
  const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
  float* out = static_cast<float*>(d->out);
  if (d->mode == 0) SDF_LAUNCH(iwe_gather_kernel<false>, grid, block, 0, s, tab, rec_s, out, g);
  else SDF_LAUNCH(iwe_gather_kernel<true>, grid, block, 0, s, tab, rec_s, out, g);
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t sdf_iwe_stats_workspace_bytes(int B, int H, int W) {
  const int64_t t = rt_tiles(B, H, W);
  return t ? (int64_t)B * t * kIsFields * 8 : 0;
}

extern "C" int sdf_iwe_stats_fwd(const SdfIweStatsDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  int64_t tiles;
  if (int rc = rt_check(d->B, d->H, d->W, d->row0, d->rows, kIsFields, {d->iwe}, d->table, d->workspace, d->workspace_bytes, tiles)) return rc;
  if (!sdf_on_device(d->iwe) || !sdf_on_device(d->table) || !sdf_on_device(d->workspace)) return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  const int hw = d->H * d->W, nblk = (int)tiles;
  SDF_LAUNCH(iwe_stats_partial_kernel, dim3(nblk, d->B), dim3(kRtThreads), 0, s, d->iwe, hw, nblk, part);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(iwe_stats_finish_kernel, dim3(d->B), dim3(64), 0, s, part, nblk, d->table + (int64_t)d->row0 * kIsFields);
  SDF_LAUNCH_CHECK();
  return 0;
}
