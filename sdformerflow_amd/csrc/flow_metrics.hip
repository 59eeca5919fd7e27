// Flow maps -> the evaluation metrics' per-sample sums, gfx950.
//
// Replaces, per sample, the element-wise and reduction launches of the reference's AEE and AAE classes (loss/flow_supervised.py
// :119-149, :163-175): one record {n_valid, sum_err, n_pe1, n_pe2, n_pe3, n_outlier, sum_ang, n_pixels} per sample, written to a row of
// a caller-owned fp64 table, so that an evaluation of any length accumulates on the device and is read back once.
//
// Per pixel every operation is a separately rounded fp32 operation in the reference's order (the build does not contract); constants
// are Python doubles rounded to fp32, as torch forms them.  Counts are integers; sum_err, sum_ang and n_valid are fp64 sums of the fp32
// per-pixel values.  No float atomics: lane -> wave -> workgroup -> one partial record per workgroup, and a second kernel adds a
// sample's partials in index order (record_table.h).  The record of a sample depends on that sample alone: two runs, or two batchings, give the same bits.
//
// Launch sequence: partial records (grid: tiles x samples) | finish (one workgroup per sample).
#include "record_table.h"

namespace {

constexpr int kFmFields = 8;

struct FmAcc {
  double n, err, ang;
  unsigned pe1, pe2, pe3, out;
};

// torch.clamp: NaN stays
__device__ __forceinline__ float fm_clamp(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(kRtThreads) void flow_metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                                          const float* __restrict__ valid, const float* __restrict__ emask,
                                                                          int hw, int nblk, float scaling, double* __restrict__ part) {
  const int b = blockIdx.y;
  const float* px = pred + (int64_t)b * 2 * hw;
  const float* lx = label + (int64_t)b * 2 * hw;
  const float* vm = valid + (int64_t)b * hw;
  const float* em = emask ? emask + (int64_t)b * hw : nullptr;
  const float eps = (float)1e-7, cmin = (float)(-1.0 + 1e-7), cmax = (float)(1.0 - 1e-7), frac = (float)0.05;
  FmAcc a = {0.0, 0.0, 0.0, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kRtPerLane; ++k) {
    const int i = blockIdx.x * kRtTile + k * kRtThreads + threadIdx.x;
    if (i >= hw) continue;
    const float fx = px[i] * scaling, fy = px[hw + i] * scaling;
    const float gx = lx[i], gy = lx[hw + i];
    float m = vm[i];
    if (em) m = m * em[i];
    const float dx = fx - gx, dy = fy - gy;
    const float e = sqrtf(dx * dx + dy * dy) * m;
    const float mag = sqrtf(fx * fx + fy * fy) * m;
    const float gm = sqrtf(gx * gx + gy * gy) * m;
    const float dot = fx * gx + fy * gy;
    const float c = fm_clamp((dot + eps) / (mag * gm + eps), cmin, cmax);
    const float ang = acosf(c) * m;
    a.n += (double)m;
    a.err += (double)e;
    a.ang += (double)ang;
    a.pe1 += e > 1.0f;
    a.pe2 += e > 2.0f;
    a.pe3 += e > 3.0f;
    a.out += (e > 3.0f) && (e > frac * mag);
  }
  const double rec[7] = {rt_wave_sum(a.n), rt_wave_sum(a.err), (double)rt_wave_sum(a.pe1), (double)rt_wave_sum(a.pe2),
                         (double)rt_wave_sum(a.pe3), (double)rt_wave_sum(a.out), rt_wave_sum(a.ang)};
  rt_block_store<7>(rec, part + ((int64_t)b * nblk + blockIdx.x) * kFmFields);
}

// sample blockIdx.x: lane k adds field k of the sample's partial records in index order; field 7 is the pixel count
__global__ __launch_bounds__(64) void flow_metrics_finish_kernel(const double* __restrict__ part, int nblk, int hw, double* __restrict__ rows) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= kFmFields) return;
  rows[(int64_t)b * kFmFields + k] = k < 7 ? rt_finish_field<kFmFields>(part + (int64_t)b * nblk * kFmFields, nblk, k) : (double)hw;
}

}  // namespace

extern "C" int64_t sdf_flow_metrics_workspace_bytes(int B, int H, int W) {
  const int64_t t = rt_tiles(B, H, W);
  return t ? (int64_t)B * t * kFmFields * 8 : 0;
}

extern "C" int sdf_flow_metrics_fwd(const SdfFlowMetricsDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  int64_t tiles;
  if (int rc = rt_check(d->B, d->H, d->W, d->row0, d->rows, kFmFields, {d->pred, d->label, d->valid}, d->table, d->workspace,
                        d->workspace_bytes, tiles))
    return rc;
  if (!sdf_aligned(d->event_mask, 4)) return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  const int hw = d->H * d->W, nblk = (int)tiles;
  SDF_LAUNCH(flow_metrics_partial_kernel, dim3(nblk, d->B), dim3(kRtThreads), 0, s, d->pred, d->label, d->valid, d->event_mask, hw, nblk,
             d->flow_scaling, part);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(flow_metrics_finish_kernel, dim3(d->B), dim3(64), 0, s, part, nblk, hw, d->table + (int64_t)d->row0 * kFmFields);
  SDF_LAUNCH_CHECK();
  return 0;
}
