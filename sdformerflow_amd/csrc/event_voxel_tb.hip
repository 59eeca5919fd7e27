// Raw event lists -> the time-bilinear voxel grid of the MVSEC / MDR loaders, gfx950.
//
// Replaces the reference's EventSequenceToVoxelGrid_Pytorch (MDR_dataloader/loader_utils.py:421-577: integer pixels, bilinear in time
// only, float64 times, two index_add_ passes, normalisation by the mean / std of the grid's own non-zeros) and, fused behind it, what
// the evaluation loop does before the model sees it (eval_MV_flow_SNN.py:162-219: old | new along the bins, polarity split, min-max
// over the non-zeros, spike threshold, event mask).
//
// The scheme is event_voxel.hip's.  No float atomics: a cell's sum is formed by ONE lane in the order the reference's CPU index_add_
// forms it - the left pass (events whose bin is the cell's) in list order, then the right pass (events of the bin before) in list
// order.  The order comes from a stable sort of the events by the key of their base cell (list, bin, y, x), which is the caller's
// (sdf_event_voxel_tb_keys_fwd writes the keys, sdf_event_voxel_tb_gather_fwd takes the sorted keys and the permutation).  The
// statistics of a list are fp64 sums over per-workgroup partials combined in a fixed order (record_table.h); min / max are integer
// atomics on bit patterns (model_input.h).  Nothing depends on arrival order: two runs, or two batchings, give the same bits.
//
// Launch sequence: keys (one launch per list) | [caller: stable sort] | clear the run table | runs + permute | gather (+ partial
// statistics) | [statistics] | [normalise / split / min-max] | [model_input.h's finish: min-max, threshold, event mask].
#include "event_common.h"
#include "model_input.h"
#include "record_table.h"

namespace {

struct TbGeom {
  int32_t L, S, nb;              // lists, lists per sample, bins per list
  int32_t H, W;                  // sensor
  int32_t h, w, oy, ox;          // output window
  int32_t dh, dw, doy, dox;      // computed window: the whole sensor when the statistics are wanted (they run over the whole grid)
  int32_t nblk;                  // gather workgroups per list
  int32_t KT;                    // number of keys = L nb dh dw; KT itself = "adds nothing"
};

// XY: 0 = fp32 coordinates, 1 = int32, 2 = uint16.  One list per launch.
template <int XY>
__global__ __launch_bounds__(256) void tb_keys_kernel(const void* __restrict__ xs, const void* __restrict__ ys, const double* __restrict__ t,
                                                      const float* __restrict__ p, double t_scale, int64_t i0, int n, int l, TbGeom g,
                                                      int* __restrict__ keys, float2* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t e = i0 + i;
  int xi = -1, yi = -1;
  if (XY == 0) {
    const float x = static_cast<const float*>(xs)[e], y = static_cast<const float*>(ys)[e];
    if (x > -1.f && x < (float)g.W && y > -1.f && y < (float)g.H) {      // .long(): truncation toward zero (NaN fails the range)
      xi = (int)x;
      yi = (int)y;
    }
  } else if (XY == 1) {
    xi = static_cast<const int32_t*>(xs)[e];
    yi = static_cast<const int32_t*>(ys)[e];
  } else {
    xi = static_cast<const uint16_t*>(xs)[e];
    yi = static_cast<const uint16_t*>(ys)[e];
  }
  // EventSequence: ts *= multiplier, ts -= ts[0]; then (nb - 1) (ts - ts[0]) / deltaT, multiply then divide - every step one fp64
  // operation (the build does not contract), and one rounding to fp32 at the end
  const double first = t[i0] * t_scale;
  const double rel = t[e] * t_scale - first;
  double delta = t[i0 + n - 1] * t_scale - first;
  if (delta == 0.0) delta = 1.0;
  const double tn = ((double)(g.nb - 1) * rel) / delta;
  const double tf = floor(tn);
  const float dts = (float)(tn - tf);
  float pol = p[e];
  if (pol == 0.f) pol = -1.f;
  int key = g.KT;
  xi -= g.dox;
  yi -= g.doy;
  if (tn >= 0.0 && tn < (double)g.nb && xi >= 0 && xi < g.dw && yi >= 0 && yi < g.dh)
    key = ((l * g.nb + (int)tf) * g.dh + yi) * g.dw + xi;
  keys[e] = key;
  rec[e] = make_float2(dts, pol);
}

// one event's term: r = (dts, pol); the left pass weights with 1 - dts, the right pass with dts, each one fp32 product with pol
template <bool POLS>
__device__ __forceinline__ void tb_add(const float2 r, int right, float& acc, float& acc2) {
  const float wt = right ? r.x : 1.0f - r.x;
  if (POLS) {
    if (r.y == 1.f) acc += wt;
    if (r.y == -1.f) acc2 += wt;
  } else {
    acc += r.y * wt;
  }
}

// tb_add of the left or the right pass (the same for every cell: event_common.h event_sum_run)
template <bool POLS>
struct TbTerm {
  int right;
  __device__ __forceinline__ void operator()(const float2 r, float& acc, float& acc2) const { tb_add<POLS>(r, right, acc, acc2); }
  __device__ __forceinline__ TbTerm of_lane(int) const { return *this; }
};

// a cell's value as the reference normalises it: non-zeros become (v - mean) / std, evaluated in fp64 and rounded once
__device__ __forceinline__ float tb_normalise(float v, const double* __restrict__ st) {
  return v != 0.f ? (float)(((double)v - st[0]) / st[1]) : v;
}

// One lane per cell of the computed window of list blockIdx.y; the raw sums go to `out` where the cell lies inside the output window:
// POLS false: at ((l nb + c) planes) h w + pixel, planes = 1 (signed volumes) or 2 (the model input's first plane; the split follows);
// POLS true: both planes of (L, nb, 2, h, w).  want_stats: count / sum / sum of squares of the non-zero values, fp64, per workgroup.
template <bool POLS>
__global__ __launch_bounds__(256) void tb_gather_kernel(const int2* __restrict__ tab, const float2* __restrict__ rec, float* __restrict__ out,
                                                        double* __restrict__ part, TbGeom g, int planes, int want_stats) {
  const int l = blockIdx.y;
  const int cells = g.nb * g.dh * g.dw;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool active = idx < cells;
  const int cell = active ? idx : 0;
  const int lane = threadIdx.x & 63;
  const int xx = cell % g.dw, yy = (cell / g.dw) % g.dh, c = cell / (g.dw * g.dh);
  float acc = 0.f, acc2 = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {                                  // left: the events of bin c; right: those of bin c - 1
    int2 r = make_int2(0, 0);
    if (active && c - pass >= 0) r = tab[l * cells + cell - pass * g.dh * g.dw];
    event_sum_run<POLS>(r, rec, lane, TbTerm<POLS>{pass}, acc, acc2);
  }
  const int oy = yy + g.doy - g.oy, ox = xx + g.dox - g.ox;
  if (active && oy >= 0 && oy < g.h && ox >= 0 && ox < g.w) {
    const int64_t hw = (int64_t)g.h * g.w, at = ((int64_t)(l * g.nb + c) * planes) * hw + (int64_t)oy * g.w + ox;
    out[at] = acc;
    if (POLS) out[at + hw] = acc2;
  }
  if (!want_stats) return;
  double cn = 0.0, sm = 0.0, sq = 0.0;
  if (active && acc != 0.f) {
    cn += 1.0;
    sm += (double)acc;
    sq += (double)acc * (double)acc;
  }
  if (POLS && active && acc2 != 0.f) {
    cn += 1.0;
    sm += (double)acc2;
    sq += (double)acc2 * (double)acc2;
  }
  const double sums[3] = {rt_wave_sum(cn), rt_wave_sum(sm), rt_wave_sum(sq)};
  rt_block_store<3>(sums, part + ((int64_t)l * g.nblk + blockIdx.x) * 3);
}

// list blockIdx.x: its workgroups' partials summed in a fixed order -> st = {mean, std}; std = 1 where the reference only subtracts
// the mean (std not > 0, or NaN for a single value), {0, 1} where there is no non-zero cell: (v - 0) / 1 = v
__global__ __launch_bounds__(256) void tb_stats_kernel(const double* __restrict__ part, int nblk, double* __restrict__ stats) {
  const int l = blockIdx.x, lane = threadIdx.x & 63;
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblk; i += 256)
    for (int k = 0; k < 3; ++k) a[k] += part[((int64_t)l * nblk + i) * 3 + k];
  for (int off = 32; off > 0; off >>= 1)
    for (int k = 0; k < 3; ++k) a[k] += __shfl_xor(a[k], off);
  __shared__ double red[4][3];
  if (lane == 0)
    for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = a[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const double s = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    const double q = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
    double mean = 0.0, sd = 1.0;
    if (n > 0.0) {
      mean = s / n;
      const double var = n > 1.0 ? (q - s * mean) / (n - 1.0) : 0.0;     // unbiased, as torch.std
      if (var > 0.0) sd = sqrt(var);
    }
    stats[2 * l] = mean;
    stats[2 * l + 1] = sd;
  }
}

// The pass over the written cells behind the gather.  SPLIT false: the per-list normalisation in place (n values).  SPLIT true: n =
// L nb h w cells; the raw sum lies in the first of the cell's two planes; normalise when asked, write relu(v) | relu(-v), and collect
// min / max of the non-zeros (model_input.h), one pair of atomics per workgroup.
template <bool SPLIT>
__global__ __launch_bounds__(256) void tb_norm_kernel(float* __restrict__ out, int64_t n, int64_t per_list, int64_t hw,
                                                      const double* __restrict__ stats, int normalize, unsigned* __restrict__ mm,
                                                      int want_minmax) {
  unsigned nlo = 0u, hi = 0u;                                            // (~min, max) over nothing
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t at = SPLIT ? (i / hw) * 2 * hw + i % hw : i;
    float v = out[at];
    if (normalize) v = tb_normalise(v, stats + 2 * (i / per_list));
    if (SPLIT) mi_split_store(v, out + at, hw, nlo, hi);
    else out[at] = v;
  }
  if (SPLIT && want_minmax) mi_minmax_commit(nlo, hi, mm);
}

struct TbPlan {
  TbGeom g;
  int64_t off_rec, off_rec_s, off_tab, off_part, off_stats, off_mm, bytes;
};

// geometry and workspace layout; false = SDF_E_SHAPE
bool tb_plan(int64_t n, int L, int nb, int H, int W, int crop_h, int crop_w, int crop_oy, int crop_ox, int normalize, TbPlan& pl) {
  if (n < 0 || n >= (1ll << 31) - 64 || L < 1 || L > 65535 || nb < 1 || H < 1 || W < 1 || crop_h < 0 || crop_w < 0) return false;
  if ((crop_h == 0) != (crop_w == 0) || crop_oy < 0 || crop_ox < 0) return false;
  if (crop_h == 0 && (crop_oy || crop_ox)) return false;
  if ((int64_t)crop_oy + crop_h > H || (int64_t)crop_ox + crop_w > W) return false;      // the window lies inside the sensor
  TbGeom& g = pl.g;
  g.L = L;
  g.S = 1;
  g.nb = nb;
  g.H = H;
  g.W = W;
  g.h = crop_h ? crop_h : H;
  g.w = crop_w ? crop_w : W;
  g.oy = crop_oy;
  g.ox = crop_ox;
  g.dh = normalize ? H : g.h;
  g.dw = normalize ? W : g.w;
  g.doy = normalize ? 0 : g.oy;
  g.dox = normalize ? 0 : g.ox;
  const int64_t cells = (int64_t)nb * g.dh * g.dw, KT = (int64_t)L * cells;
  if (KT >= (1ll << 31) - 256 || (int64_t)L * nb * 2 * g.h * g.w >= (1ll << 40)) return false;
  g.KT = (int)KT;
  g.nblk = (int)((cells + 255) / 256);
  pl.off_rec = 0;
  pl.off_rec_s = pl.off_rec + pad256(n * 8);
  pl.off_tab = pl.off_rec_s + pad256(n * 8);
  pl.off_part = pl.off_tab + pad256(KT * 8);
  pl.off_stats = pl.off_part + (normalize ? pad256((int64_t)L * g.nblk * 24) : 0);
  pl.off_mm = pl.off_stats + pad256((int64_t)L * 16);
  pl.bytes = pl.off_mm + 256;
  return true;
}

int tb_check(const SdfEventVoxelTbDesc* d, TbPlan& pl) {
  if (!d) return SDF_E_NULL;
  if (!tb_plan(d->n_events, d->n_lists, d->nb, d->H, d->W, d->crop_h, d->crop_w, d->crop_oy, d->crop_ox, d->normalize != 0, pl))
    return SDF_E_SHAPE;
  if (d->lists_per_sample < 1 || d->lists_per_sample > 2 || d->n_lists % d->lists_per_sample) return SDF_E_SHAPE;
  pl.g.S = d->lists_per_sample;
  if (d->mode < 0 || d->mode > 2 || d->norm < 0 || d->norm > 1 || d->xy_dtype < 0 || d->xy_dtype > 2 || d->normalize < 0 || d->normalize > 1)
    return SDF_E_DTYPE;
  // min-max, threshold and event mask belong to the model-input form; so does pairing old | new
  if (d->mode != 1 && (d->norm || d->use_spike_th || d->event_mask || d->lists_per_sample != 1)) return SDF_E_DTYPE;
  if (!d->workspace || !d->out || !d->offsets) return SDF_E_NULL;
  if (d->workspace_bytes < pl.bytes) return SDF_E_SHAPE;
  if (!sdf_aligned(d->workspace, 16) || !sdf_aligned(d->out, 4) || !sdf_aligned(d->event_mask, 4)) return SDF_E_ALIGN;
  if (!event_offsets_ok(d->offsets, d->n_lists, d->n_events)) return SDF_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int64_t sdf_event_voxel_tb_workspace_bytes(int64_t n_events, int n_lists, int nb, int H, int W, int crop_h, int crop_w,
                                                      int crop_oy, int crop_ox, int normalize) {
  TbPlan pl;
  return tb_plan(n_events, n_lists, nb, H, W, crop_h, crop_w, crop_oy, crop_ox, normalize != 0, pl) ? pl.bytes : 0;
}

extern "C" int sdf_event_voxel_tb_keys_fwd(const SdfEventVoxelTbDesc* d, void* stream) {
  TbPlan pl;
  if (int rc = tb_check(d, pl)) return rc;
  if (d->n_events == 0) return 0;
  if (int rc = event_keys_check(d->x, d->y, d->t, d->p, d->keys, d->xy_dtype, 8, false, nullptr, 0, 0)) return rc;
  const double t_scale = d->t_scale ? *d->t_scale : 1.0;
  hipStream_t s = sdf_stream(stream);
  float2* rec = reinterpret_cast<float2*>(static_cast<char*>(d->workspace) + pl.off_rec);
  return event_keys_launch(d->offsets, d->n_lists, d->xy_dtype, [&](auto xy, dim3 grid, int64_t i0, int n, int l) {
    SDF_LAUNCH(tb_keys_kernel<decltype(xy)::value>, grid, dim3(256), 0, s, d->x, d->y, d->t, d->p, t_scale, i0, n, l, pl.g, d->keys, rec);
  });
}

extern "C" int sdf_event_voxel_tb_gather_fwd(const SdfEventVoxelTbDesc* d, void* stream) {
  TbPlan pl;
  if (int rc = tb_check(d, pl)) return rc;
  const int n = (int)d->n_events;
  hipStream_t s = sdf_stream(stream);
  char* ws = static_cast<char*>(d->workspace);
  const float2* rec = reinterpret_cast<const float2*>(ws + pl.off_rec);
  float2* rec_s = reinterpret_cast<float2*>(ws + pl.off_rec_s);
  int2* tab = reinterpret_cast<int2*>(ws + pl.off_tab);
  double* part = reinterpret_cast<double*>(ws + pl.off_part);
  double* stats = reinterpret_cast<double*>(ws + pl.off_stats);
  unsigned* mm = reinterpret_cast<unsigned*>(ws + pl.off_mm);
  const TbGeom& g = pl.g;
  if (int rc = event_runs_launch(d->keys_sorted, d->order, rec, rec_s, tab, n, g.KT, s)) return rc;
  if (d->norm)
    if (int rc = mi_clear_pairs(mm, 1, s)) return rc;
  const dim3 block(256), ggrid(g.nblk, g.L);
  float* out = static_cast<float*>(d->out);
  if (d->mode == 2) SDF_LAUNCH(tb_gather_kernel<true>, ggrid, block, 0, s, tab, rec_s, out, part, g, 2, d->normalize);
  else SDF_LAUNCH(tb_gather_kernel<false>, ggrid, block, 0, s, tab, rec_s, out, part, g, d->mode == 1 ? 2 : 1, d->normalize);
  SDF_LAUNCH_CHECK();
  if (d->normalize) {
    SDF_LAUNCH(tb_stats_kernel, dim3(g.L), block, 0, s, part, g.nblk, stats);
    SDF_LAUNCH_CHECK();
  }
  const int64_t hw = (int64_t)g.h * g.w, cells = (int64_t)g.L * g.nb * hw;
  const auto blocks = [](int64_t m) { return dim3((unsigned)((m + 255) / 256 < 1024 ? (m + 255) / 256 : 1024)); };
  if (d->mode == 1) {
    SDF_LAUNCH(tb_norm_kernel<true>, blocks(cells), block, 0, s, out, cells, (int64_t)g.nb * hw, hw, stats, d->normalize, mm, d->norm);
    SDF_LAUNCH_CHECK();
    if (int rc = mi_finish(out, static_cast<float*>(d->event_mask), nullptr, g.L / g.S, (int)hw, 2 * g.S * g.nb, mm, d->norm, 0,
                           d->use_spike_th, d->spike_th, s))
      return rc;
  } else if (d->normalize) {
    const int64_t per_list = (int64_t)g.nb * hw * (d->mode == 2 ? 2 : 1);
    SDF_LAUNCH(tb_norm_kernel<false>, blocks(g.L * per_list), block, 0, s, out, g.L * per_list, per_list, hw, stats, 1, mm, 0);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}
