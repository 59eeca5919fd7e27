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
// Launch sequence: keys (one launch per list) | [caller: stable sort] | clear the run table | runs (+ permute) | gather.
//
// sdf_iwe_stats_fwd: per sample {sum c, sum c^2, max c, pixels with c != 0} of c = the fp64 sum of a pixel's two channels, as
// flow_metrics.hip forms its sums: lane -> wave -> workgroup -> one fp64 partial record per workgroup, then added in index order.
// The Flow Warp Loss (Stoffregen et al. 2020) of a sample is var(S) / var(Z) on nearest images, S warped by the flow and Z by none, with
// var = (sum c^2 - (sum c)^2 / N) / (N - 1) in fp64 over the N = h w pixels: the sums are integers, exact while below 2^53.
#include "event_common.h"

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

// XY: 0 = fp32 coordinates as given, 1 = int32 sensor coordinates through the rectify map, 2 = uint16 likewise.  NEAREST: no record.
template <int XY, bool NEAREST>
__global__ __launch_bounds__(256) void iwe_keys_kernel(const void* __restrict__ xs, const void* __restrict__ ys, const float* __restrict__ t,
                                                       const float* __restrict__ p, const float* __restrict__ flow,
                                                       const float* __restrict__ map, int map_h, int map_w, int64_t i0, int n, int b,
                                                       IweGeom g, IweParams q, int* __restrict__ keys, float2* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e = i0 + i;
  float x, y;
  bool ok = true;
  if (XY == 0) {
    x = static_cast<const float*>(xs)[e];
    y = static_cast<const float*>(ys)[e];
  } else {
    int xi, yi;
    if (XY == 1) {
      xi = static_cast<const int32_t*>(xs)[e];
      yi = static_cast<const int32_t*>(ys)[e];
    } else {
      xi = static_cast<const uint16_t*>(xs)[e];
      yi = static_cast<const uint16_t*>(ys)[e];
    }
    ok = xi >= 0 && xi < map_w && yi >= 0 && yi < map_h;        // (as event_voxel.hip: such an event adds nothing)
    const int64_t m = ok ? ((int64_t)yi * map_w + xi) * 2 : 0;
    x = map[m];
    y = map[m + 1];
  }
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

// the run table alone (nearest mode: a cell's value is its run's length, no record moves)
__global__ __launch_bounds__(256) void iwe_runs_kernel(const int* __restrict__ ks, int n, int KT, int2* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = ks[i];
  if (k < 0 || k >= KT) return;
  if (i == 0 || ks[i - 1] != k) tab[k].x = i;
  if (i == n - 1 || ks[i + 1] != k) tab[k].y = i + 1;
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
  offs = d->offsets;
  if (!offs) {
    if (d->B != 1) return SDF_E_NULL;
    own[0] = 0;
    own[1] = d->n_events;
    offs = own;
  }
  if (!event_offsets_ok(offs, d->B, d->n_events)) return SDF_E_SHAPE;
  if (d->t_range)
    for (int b = 0; b < d->B; ++b)                                       // a list whose first and last time are equal has no tn
      if (offs[b + 1] > offs[b] && !(d->t_range[2 * b + 1] != d->t_range[2 * b])) return SDF_E_SHAPE;
  return 0;
}

constexpr int kIsThreads = 256;
constexpr int kIsPerLane = 4;                           // pixels per lane, kIsThreads apart (coalesced)
constexpr int kIsTile = kIsThreads * kIsPerLane;        // pixels per workgroup
constexpr int kIsFields = 4;

__global__ __launch_bounds__(kIsThreads) void iwe_stats_partial_kernel(const float* __restrict__ iwe, int hw, int nblk,
                                                                       double* __restrict__ part) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const float* c0 = iwe + (int64_t)b * 2 * hw;
  double s1 = 0.0, s2 = 0.0, mx = 0.0;
  unsigned nz = 0u;
#pragma unroll
  for (int k = 0; k < kIsPerLane; ++k) {
    const int i = blockIdx.x * kIsTile + k * kIsThreads + threadIdx.x;
    if (i >= hw) continue;
    const double c = (double)c0[i] + (double)c0[hw + i];
    s1 += c;
    s2 += c * c;
    mx = fmax(mx, c);
    nz += c != 0.0;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
    mx = fmax(mx, __shfl_xor(mx, off));
    nz += (unsigned)__shfl_xor((int)nz, off);
  }
  __shared__ double red[kIsThreads / 64][kIsFields];
  if (lane == 0) {
    double* r = red[threadIdx.x >> 6];
    r[0] = s1;
    r[1] = s2;
    r[2] = mx;
    r[3] = (double)nz;
  }
  __syncthreads();
  if (threadIdx.x < kIsFields) {
    const int k = threadIdx.x;
    const double v = k == 2 ? fmax(fmax(red[0][k], red[1][k]), fmax(red[2][k], red[3][k]))
                            : ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    part[((int64_t)b * nblk + blockIdx.x) * kIsFields + k] = v;
  }
}

// sample blockIdx.x: lane k combines field k of the sample's partial records in index order
__global__ __launch_bounds__(64) void iwe_stats_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ rows) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= kIsFields) return;
  const double* p = part + (int64_t)b * nblk * kIsFields + k;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) {
    const double v = p[(int64_t)i * kIsFields];
    s = k == 2 ? fmax(s, v) : s + v;
  }
  rows[(int64_t)b * kIsFields + k] = s;
}

// tiles per sample; 0 = refused geometry
inline int64_t iwe_stats_tiles(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1) return 0;
  const int64_t hw = (int64_t)H * W;
  if (hw >= (1ll << 30)) return 0;
  return (hw + kIsTile - 1) / kIsTile;
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
  if (!d->x || !d->y || !d->t || !d->p || !d->keys) return SDF_E_NULL;
  if (d->xy_dtype != 0 && (!d->rectify_map || d->map_h < 1 || d->map_w < 1)) return d->rectify_map ? SDF_E_SHAPE : SDF_E_NULL;
  if (d->xy_dtype == 0 && d->rectify_map) return SDF_E_DTYPE;            // the map is indexed by integer sensor coordinates
  if (!sdf_aligned(d->x, d->xy_dtype == 2 ? 2 : 4) || !sdf_aligned(d->y, d->xy_dtype == 2 ? 2 : 4) || !sdf_aligned(d->t, 4) ||
      !sdf_aligned(d->p, 4) || !sdf_aligned(d->keys, 4) || (d->rectify_map && !sdf_aligned(d->rectify_map, 4)))
    return SDF_E_ALIGN;
  for (const void* ptr : {d->x, d->y, (const void*)d->t, (const void*)d->p, (const void*)d->flow, (const void*)d->keys,
                          (const void*)d->workspace})
    if (!sdf_on_device(ptr)) return SDF_E_DTYPE;
  if (d->rectify_map && !sdf_on_device(d->rectify_map)) return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  float2* rec = reinterpret_cast<float2*>(static_cast<char*>(d->workspace) + pl.off_rec);
  const IweParams q = {d->scale, d->t_ref, d->win_a, d->win_b};
  for (int b = 0; b < d->B; ++b) {
    const int64_t i0 = offs[b];
    const int n = (int)(offs[b + 1] - i0);
    if (n == 0) continue;
    const dim3 grid((n + 255) / 256), block(256);
#define IWE_KEYS(XY, NEAREST)                                                                                                          \
  SDF_LAUNCH((iwe_keys_kernel<XY, NEAREST>), grid, block, 0, s, d->x, d->y, d->t, d->p, d->flow, d->rectify_map, d->map_h, d->map_w, i0, \
             n, b, pl.g, q, d->keys, rec)
    if (d->mode == 0) {
      if (d->xy_dtype == 0) IWE_KEYS(0, false);
      else if (d->xy_dtype == 1) IWE_KEYS(1, false);
      else IWE_KEYS(2, false);
    } else {
      if (d->xy_dtype == 0) IWE_KEYS(0, true);
      else if (d->xy_dtype == 1) IWE_KEYS(1, true);
      else IWE_KEYS(2, true);
    }
#undef IWE_KEYS
    SDF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int sdf_event_iwe_gather_fwd(const SdfEventIweDesc* d, void* stream) {
  IwePlan pl;
  const int64_t* offs;
  int64_t own[2];
  if (int rc = iwe_check(d, pl, offs, own)) return rc;
  const int n = (int)d->n_events;
  if (n && (!d->keys_sorted || !d->order)) return SDF_E_NULL;
  if (n && (!sdf_aligned(d->keys_sorted, 4) || !sdf_aligned(d->order, 8))) return SDF_E_ALIGN;
  if (!sdf_on_device(d->out) || !sdf_on_device(d->workspace) || (n && (!sdf_on_device(d->keys_sorted) || !sdf_on_device(d->order))))
    return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  char* ws = static_cast<char*>(d->workspace);
  const float2* rec = reinterpret_cast<const float2*>(ws + pl.off_rec);
  float2* rec_s = reinterpret_cast<float2*>(ws + pl.off_rec_s);
  int2* tab = reinterpret_cast<int2*>(ws + pl.off_tab);
  const IweGeom& g = pl.g;
  if (d->mode == 0) {
    if (int rc = event_runs_launch(d->keys_sorted, d->order, rec, rec_s, tab, (unsigned*)nullptr, n, g.KT, 0, s)) return rc;
  } else {
    hipError_t e = hipMemsetAsync(tab, 0, (size_t)g.KT * 8, s);          // every run empty
    if (e != hipSuccess) return (int)e;
    if (n) {
      SDF_LAUNCH(iwe_runs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d->keys_sorted, n, g.KT, tab);
      SDF_LAUNCH_CHECK();
    }
  }
  const int64_t cells = (int64_t)g.B * 2 * g.h * g.w;
  const dim3 grid((unsigned)((cells + 255) / 256)), block(256);
  float* out = static_cast<float*>(d->out);
  if (d->mode == 0) SDF_LAUNCH(iwe_gather_kernel<false>, grid, block, 0, s, tab, rec_s, out, g);
  else SDF_LAUNCH(iwe_gather_kernel<true>, grid, block, 0, s, tab, rec_s, out, g);
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t sdf_iwe_stats_workspace_bytes(int B, int H, int W) {
  const int64_t t = iwe_stats_tiles(B, H, W);
  return t ? (int64_t)B * t * kIsFields * 8 : 0;
}

extern "C" int sdf_iwe_stats_fwd(const SdfIweStatsDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  const int64_t tiles = iwe_stats_tiles(d->B, d->H, d->W);
  if (!tiles) return SDF_E_SHAPE;
  if (d->row0 < 0 || (int64_t)d->row0 + d->B > d->rows) return SDF_E_SHAPE;       // the records lie inside the table
  if (!d->iwe || !d->table || !d->workspace) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)d->B * tiles * kIsFields * 8) return SDF_E_SHAPE;
  if (!sdf_aligned(d->iwe, 4) || !sdf_aligned(d->table, 8) || !sdf_aligned(d->workspace, 8)) return SDF_E_ALIGN;
  if (!sdf_on_device(d->iwe) || !sdf_on_device(d->table) || !sdf_on_device(d->workspace)) return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  const int hw = d->H * d->W, nblk = (int)tiles;
  SDF_LAUNCH(iwe_stats_partial_kernel, dim3(nblk, d->B), dim3(kIsThreads), 0, s, d->iwe, hw, nblk, part);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(iwe_stats_finish_kernel, dim3(d->B), dim3(64), 0, s, part, nblk, d->table + (int64_t)d->row0 * kIsFields);
  SDF_LAUNCH_CHECK();
  return 0;
}
