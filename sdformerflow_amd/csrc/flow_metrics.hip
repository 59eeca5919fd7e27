// Flow maps -> the evaluation metrics' per-sample sums, gfx950.
//
// Replaces, per sample, the element-wise and reduction launches of the reference's AEE and AAE classes (loss/flow_supervised.py
// :119-149, :163-175): one record {n_valid, sum_err, n_pe1, n_pe2, n_pe3, n_outlier, sum_ang, n_pixels} per sample, written to a row of
// a caller-owned fp64 table, so that an evaluation of any length accumulates on the device and is read back once.
//
// Per pixel every operation is a separately rounded fp32 operation in the reference's order (the build does not contract); constants
// are Python doubles rounded to fp32, as torch forms them.  Counts are integers; sum_err, sum_ang and n_valid are fp64 sums of the fp32
// per-pixel values.  No float atomics: lane -> wave -> workgroup -> one partial record per workgroup, and a second kernel adds a
// sample's partials in index order.  The record of a sample depends on that sample alone: two runs, or two batchings, give the same bits.
//
// Launch sequence: partial records (grid: tiles x samples) | finish (one workgroup per sample).
#include "common.h"

namespace {

constexpr int kFmThreads = 256;
constexpr int kFmPerLane = 4;                           // pixels per lane, kFmThreads apart (coalesced)
constexpr int kFmTile = kFmThreads * kFmPerLane;        // pixels per workgroup
constexpr int kFmFields = 8;

struct FmAcc {
  double n, err, ang;
  unsigned pe1, pe2, pe3, out;
};

// torch.clamp: NaN stays
__device__ __forceinline__ float fm_clamp(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

__global__ __launch_bounds__(kFmThreads) void flow_metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                                          const float* __restrict__ valid, const float* __restrict__ emask,
                                                                          int hw, int nblk, float scaling, double* __restrict__ part) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const float* px = pred + (int64_t)b * 2 * hw;
  const float* lx = label + (int64_t)b * 2 * hw;
  const float* vm = valid + (int64_t)b * hw;
  const float* em = emask ? emask + (int64_t)b * hw : nullptr;
  const float eps = (float)1e-7, cmin = (float)(-1.0 + 1e-7), cmax = (float)(1.0 - 1e-7), frac = (float)0.05;
  FmAcc a = {0.0, 0.0, 0.0, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kFmPerLane; ++k) {
    const int i = blockIdx.x * kFmTile + k * kFmThreads + threadIdx.x;
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
  for (int off = 32; off > 0; off >>= 1) {
    a.n += __shfl_xor(a.n, off);
    a.err += __shfl_xor(a.err, off);
    a.ang += __shfl_xor(a.ang, off);
    a.pe1 += (unsigned)__shfl_xor((int)a.pe1, off);
    a.pe2 += (unsigned)__shfl_xor((int)a.pe2, off);
    a.pe3 += (unsigned)__shfl_xor((int)a.pe3, off);
    a.out += (unsigned)__shfl_xor((int)a.out, off);
  }
  __shared__ double red[kFmThreads / 64][7];
  if (lane == 0) {
    double* r = red[threadIdx.x >> 6];
    r[0] = a.n;
    r[1] = a.err;
    r[2] = (double)a.pe1;
    r[3] = (double)a.pe2;
    r[4] = (double)a.pe3;
    r[5] = (double)a.out;
    r[6] = a.ang;
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int k = threadIdx.x;
    part[((int64_t)b * nblk + blockIdx.x) * kFmFields + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// sample blockIdx.x: lane k adds field k of the sample's partial records in index order; field 7 is the pixel count
__global__ __launch_bounds__(64) void flow_metrics_finish_kernel(const double* __restrict__ part, int nblk, int hw, double* __restrict__ rows) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= kFmFields) return;
  double s = 0.0;
  if (k < 7) {
    const double* p = part + (int64_t)b * nblk * kFmFields + k;
    for (int i = 0; i < nblk; ++i) s += p[(int64_t)i * kFmFields];
  } else {
    s = (double)hw;
  }
  rows[(int64_t)b * kFmFields + k] = s;
}

// tiles per sample; 0 = refused geometry
inline int64_t fm_tiles(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1) return 0;
  const int64_t hw = (int64_t)H * W;
  if (hw >= (1ll << 30)) return 0;                       // pixel indices and 2 hw stay inside 31 bits
  return (hw + kFmTile - 1) / kFmTile;
}

}  // namespace

extern "C" int64_t sdf_flow_metrics_workspace_bytes(int B, int H, int W) {
  const int64_t t = fm_tiles(B, H, W);
  return t ? (int64_t)B * t * kFmFields * 8 : 0;
}

extern "C" int sdf_flow_metrics_fwd(const SdfFlowMetricsDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  const int64_t tiles = fm_tiles(d->B, d->H, d->W);
  if (!tiles) return SDF_E_SHAPE;
  if (d->row0 < 0 || (int64_t)d->row0 + d->B > d->rows) return SDF_E_SHAPE;       // the records lie inside the table
  if (!d->pred || !d->label || !d->valid || !d->table || !d->workspace) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)d->B * tiles * kFmFields * 8) return SDF_E_SHAPE;
  if (!sdf_aligned(d->pred, 4) || !sdf_aligned(d->label, 4) || !sdf_aligned(d->valid, 4) || !sdf_aligned(d->event_mask, 4) ||
      !sdf_aligned(d->table, 8) || !sdf_aligned(d->workspace, 8))
    return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  const int hw = d->H * d->W, nblk = (int)tiles;
  SDF_LAUNCH(flow_metrics_partial_kernel, dim3(nblk, d->B), dim3(kFmThreads), 0, s, d->pred, d->label, d->valid, d->event_mask, hw, nblk,
             d->flow_scaling, part);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(flow_metrics_finish_kernel, dim3(d->B), dim3(64), 0, s, part, nblk, hw, d->table + (int64_t)d->row0 * kFmFields);
  SDF_LAUNCH_CHECK();
  return 0;
}
