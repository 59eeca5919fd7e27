// Decoder predictions of every level -> the supervised multi-scale flow loss and its gradient at each level's own resolution, gfx950.
//
// Replaces, per training step, forward_train's `pred.sum(0)` + F.interpolate per level and flow_loss_supervised's element-wise and
// reduction launches (reference loss/flow_supervised.py:85-102, gamma None) together with their autograd twins: no (B, 2, H, W)
// tensor per level exists in either direction.  Level i, factor s = H / h = W / w in {1, 2, 4, 8, 16} - the factors at which
// F.interpolate's nearest index floor(dst * (1 / s)) in fp32 is dst / s - at full-resolution pixel (Y, X) of sample b:
//   f = sum_t pred[t][b][c][Y / s][X / s]  (fp32, t ascending; 16-bit inputs: rounded once to the input type when T > 1)
//   d = f * fs - label;  r = sqrtf(dx * dx + dy * dy + 1e-8f);  err = r * m
//   S[i][b] = sum err  (fp64 sum of the fp32 values);  loss = mean_b sum_i lambda S[i][b] / (n + 1e-9f) / levels  (fp64, rounded once)
//   grad[i][b][c][y][x] = sum over the s x s block, row-major, of  m * d_c / r * (fs lambda / (levels B) / (n + 1e-9f))
// Every operation is rounded on its own (the build does not contract); constants are Python doubles rounded to fp32.  The mask
// multiplies, it does not select: a non-finite prediction under a zero mask gives NaN, as the torch composition does.
//
// A workgroup owns a 16-row x 64-column tile of the full-resolution frame, aligned to 16, so every s x s block lies inside one
// workgroup: each gradient element is written once, by one thread, from an LDS tile of the per-pixel terms added in a fixed order.  Each
// thread reads label and mask of its 4 pixels once and loops over the levels.  Loss partials go lane -> wave -> workgroup -> one fp64 per
// (sample, tile, level) in the workspace; the finish kernel adds them in index order.  No float atomics; the same bits on every run; a
// sample's record depends on that sample alone.
//
// Launch sequence: partial (grid: tiles x samples) | finish (one workgroup), whatever the number of levels.
#include "common.h"

namespace {

constexpr int kFlThreads = 256;
constexpr int kFlTileH = 16, kFlTileW = 64;             // rows x columns of a workgroup's tile; 4 rows per lane, kFlThreads / kFlTileW apart
constexpr int kFlPerLane = kFlTileH * kFlTileW / kFlThreads;
constexpr int kFlMaxLevels = SDF_FLOW_LOSS_MAX_LEVELS;
constexpr int kFlMaxLowres = 2 * (kFlTileH / 2) * (kFlTileW / 2);       // f values under a tile at factor 2, both components

struct FlLevels {                                       // the partial kernel's per-level arguments
  const void* pred[kFlMaxLevels];
  float* grad[kFlMaxLevels];
  int h[kFlMaxLevels], w[kFlMaxLevels], T[kFlMaxLevels], ls[kFlMaxLevels];      // ls = log2(factor)
};

template <int DT>
__device__ __forceinline__ float fl_load(const void* p, int64_t i) {
  if (DT == SDF_FLOW_LOSS_F32) return static_cast<const float*>(p)[i];
  if (DT == SDF_FLOW_LOSS_BF16) return __uint_as_float((uint32_t) static_cast<const uint16_t*>(p)[i] << 16);
  return (float)static_cast<const _Float16*>(p)[i];
}

// fp32 -> the input type and back, round to nearest even (NaN stays NaN)
template <int DT>
__device__ __forceinline__ float fl_round(float f) {
  if (DT == SDF_FLOW_LOSS_F32) return f;
  if (DT == SDF_FLOW_LOSS_F16) return (float)(_Float16)f;
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return f;
  u += 0x7fffu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xffff0000u);
}

// f of one level pixel: pred[t] at `first` + t * step, t ascending
template <int DT>
__device__ __forceinline__ float fl_sum_t(const void* pred, int T, int64_t first, int64_t step) {
  float f = fl_load<DT>(pred, first);
  for (int t = 1; t < T; ++t) f += fl_load<DT>(pred, first + t * step);
  return T > 1 ? fl_round<DT>(f) : f;
}

template <int DT>
__global__ __launch_bounds__(kFlThreads) void flow_loss_partial_kernel(FlLevels L, const float* __restrict__ label,
                                                                       const float* __restrict__ mask, const float* __restrict__ n_valid,
                                                                       int levels, int B, int H, int W, int tiles_x, float fs, float c0,
                                                                       double* __restrict__ part) {
  __shared__ float gt[2][kFlTileH][kFlTileW];           // the level's per-pixel gradient terms (factors >= 2)
  __shared__ float ft[kFlMaxLowres];                    // f of the level's pixels under the tile (factors >= 2)
  __shared__ double red[kFlThreads / 64][kFlMaxLevels];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int col = tid & 63, wave = tid >> 6;
  const int X = tx * kFlTileW + col;
  const int64_t hw = (int64_t)H * W;
  const bool want_grad = L.grad[0] != nullptr;
  float lx[kFlPerLane], ly[kFlPerLane], m[kFlPerLane];
  bool in[kFlPerLane];
#pragma unroll
  for (int k = 0; k < kFlPerLane; ++k) {
    const int Y = ty * kFlTileH + wave + 4 * k;
    in[k] = Y < H && X < W;
    lx[k] = ly[k] = m[k] = 0.f;
    if (in[k]) {
      const int64_t p = (int64_t)Y * W + X;
      lx[k] = label[(int64_t)b * 2 * hw + p];
      ly[k] = label[((int64_t)b * 2 + 1) * hw + p];
      m[k] = mask[(int64_t)b * hw + p];
    }
  }
  const float eps = (float)1e-8;
  const float kf = c0 / (*n_valid + (float)1e-9);       // fs lambda / (levels B) / (n + 1e-9)
  for (int lvl = 0; lvl < levels; ++lvl) {
    const void* pred = L.pred[lvl];
    float* grad = L.grad[lvl];
    const int ls = L.ls[lvl], h = L.h[lvl], w = L.w[lvl], T = L.T[lvl];
    const int64_t plane = (int64_t)h * w, tstep = (int64_t)B * 2 * plane, base = (int64_t)b * 2 * plane;
    const int tw = kFlTileW >> ls, n_low = (kFlTileH >> ls) * tw;                 // the tile in the level's pixels
    const int ly0 = (ty * kFlTileH) >> ls, lx0 = (tx * kFlTileW) >> ls;
    if (ls > 0) {
      __syncthreads();                                  // the previous level's reads of ft and gt are done
      for (int idx = tid; idx < 2 * n_low; idx += kFlThreads) {
        const int c = idx >= n_low, r = idx - c * n_low;
        const int y = ly0 + r / tw, x = lx0 + r % tw;
        if (y < h && x < w) ft[idx] = fl_sum_t<DT>(pred, T, base + c * plane + (int64_t)y * w + x, tstep);
      }
      __syncthreads();
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kFlPerLane; ++k) {
      const int row = wave + 4 * k;
      float gx = 0.f, gy = 0.f;
      if (in[k]) {
        float fx, fy;
        if (ls == 0) {
          const int64_t i = base + (int64_t)(ty * kFlTileH + row) * w + X;
          fx = fl_sum_t<DT>(pred, T, i, tstep);
          fy = fl_sum_t<DT>(pred, T, i + plane, tstep);
        } else {
          const int r = (row >> ls) * tw + (col >> ls);
          fx = ft[r];
          fy = ft[n_low + r];
        }
        const float dx = fx * fs - lx[k], dy = fy * fs - ly[k];
        const float r = sqrtf(dx * dx + dy * dy + eps);
        acc += (double)(r * m[k]);
        if (want_grad) {
          gx = m[k] * dx / r * kf;
          gy = m[k] * dy / r * kf;
          if (ls == 0) {
            const int64_t i = base + (int64_t)(ty * kFlTileH + row) * w + X;
            grad[i] = gx;
            grad[i + plane] = gy;
          }
        }
      }
      if (want_grad && ls > 0) {
        gt[0][row][col] = gx;
        gt[1][row][col] = gy;
      }
    }
    if (want_grad && ls > 0) {
      __syncthreads();
      const int s = 1 << ls;
      for (int idx = tid; idx < 2 * n_low; idx += kFlThreads) {                   // one thread per s x s block and component
        const int c = idx >= n_low, r = idx - c * n_low;
        const int yl = r / tw, xl = r % tw;
        const int y = ly0 + yl, x = lx0 + xl;
        if (y < h && x < w) {
          float g = 0.f;
          for (int yy = 0; yy < s; ++yy)
            for (int xx = 0; xx < s; ++xx) g += gt[c][yl * s + yy][xl * s + xx];
          grad[base + c * plane + (int64_t)y * w + x] = g;
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (col == 0) red[wave][lvl] = acc;
  }
  __syncthreads();
  if (tid < levels)
    part[((int64_t)b * gridDim.x + tile) * levels + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one workgroup: thread k adds the partials of (level, sample) pairs k, k + 256, ... in index order, records them, and the pairs'
// terms lambda S / (n + 1e-9) are added thread by thread and then down a fixed tree
__global__ __launch_bounds__(kFlThreads) void flow_loss_finish_kernel(const double* __restrict__ part, int tiles, int levels, int B,
                                                                      const float* __restrict__ n_valid, float lambda_mod,
                                                                      double* __restrict__ records, float* __restrict__ loss) {
  __shared__ double red[kFlThreads];
  const double np = (double)(*n_valid + (float)1e-9), lam = (double)lambda_mod;
  double acc = 0.0;
  for (int k = threadIdx.x; k < levels * B; k += kFlThreads) {
    const int lvl = k / B, b = k - lvl * B;
    const double* p = part + (int64_t)b * tiles * levels + lvl;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < tiles; ++i) s += p[(int64_t)i * levels];      // (index order; unrolled so that the loads do not wait for the sums)
    if (records) records[k] = s;
    acc += lam * s / np;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = kFlThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] / (double)levels / (double)B);
}

// tiles per sample; 0 = refused geometry
inline int64_t fl_tiles(int B, int H, int W, int levels) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || levels < 1 || levels > kFlMaxLevels) return 0;
  if ((int64_t)H * W >= (1ll << 30)) return 0;           // pixel indices and 2 H W stay inside 31 bits
  return (int64_t)((H + kFlTileH - 1) / kFlTileH) * ((W + kFlTileW - 1) / kFlTileW);
}

}  // namespace

extern "C" int64_t sdf_flow_loss_workspace_bytes(int B, int H, int W, int levels) {
  return (int64_t)B * fl_tiles(B, H, W, levels) * levels * 8;
}

extern "C" int sdf_flow_loss_fwd(const SdfFlowLossDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (d->levels < 1 || d->levels > kFlMaxLevels) return SDF_E_SHAPE;
  const int64_t tiles = fl_tiles(d->B, d->H, d->W, d->levels);
  if (!tiles) return SDF_E_SHAPE;
  if (d->dtype != SDF_FLOW_LOSS_F32 && d->dtype != SDF_FLOW_LOSS_BF16 && d->dtype != SDF_FLOW_LOSS_F16) return SDF_E_DTYPE;
  if (!d->label || !d->mask || !d->n_valid || !d->loss || !d->workspace) return SDF_E_NULL;
  const size_t pred_align = d->dtype == SDF_FLOW_LOSS_F32 ? 4 : 2;
  FlLevels L;
  for (int i = 0; i < kFlMaxLevels; ++i) {
    L.pred[i] = nullptr;
    L.grad[i] = nullptr;
    L.h[i] = L.w[i] = L.T[i] = L.ls[i] = 0;
  }
  for (int i = 0; i < d->levels; ++i) {
    const int h = d->h[i], w = d->w[i];
    if (!d->pred[i]) return SDF_E_NULL;
    if ((d->grad[i] != nullptr) != (d->grad[0] != nullptr)) return SDF_E_NULL;      // gradients for every level or for none
    if (d->T[i] < 1 || d->T[i] > 64 || h < 1 || w < 1 || d->H % h || d->W % w) return SDF_E_SHAPE;
    const int s = d->H / h;
    if (s != d->W / w) return SDF_E_SHAPE;                                           // square factors
    int ls = 0;
    while ((1 << ls) < s) ++ls;
    if ((1 << ls) != s || s > kFlTileH) return SDF_E_SHAPE;                          // 1, 2, 4, 8, 16
    if (!sdf_aligned(d->pred[i], pred_align) || !sdf_aligned(d->grad[i], 4)) return SDF_E_ALIGN;
    L.pred[i] = d->pred[i];
    L.grad[i] = d->grad[i];
    L.h[i] = h;
    L.w[i] = w;
    L.T[i] = d->T[i];
    L.ls[i] = ls;
  }
  if (d->workspace_bytes < (int64_t)d->B * tiles * d->levels * 8) return SDF_E_SHAPE;
  if (!sdf_aligned(d->label, 4) || !sdf_aligned(d->mask, 4) || !sdf_aligned(d->n_valid, 4) || !sdf_aligned(d->loss, 4) ||
      !sdf_aligned(d->records, 8) || !sdf_aligned(d->workspace, 8))
    return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  const int tiles_x = (d->W + kFlTileW - 1) / kFlTileW;
  const float c0 = (float)((double)d->flow_scaling * (double)d->lambda_mod / ((double)d->levels * (double)d->B));
  const dim3 grid((unsigned)tiles, d->B);
  if (d->dtype == SDF_FLOW_LOSS_F32) {
    SDF_LAUNCH(flow_loss_partial_kernel<SDF_FLOW_LOSS_F32>, grid, dim3(kFlThreads), 0, s, L, d->label, d->mask, d->n_valid, d->levels, d->B,
               d->H, d->W, tiles_x, d->flow_scaling, c0, part);
  } else if (d->dtype == SDF_FLOW_LOSS_BF16) {
    SDF_LAUNCH(flow_loss_partial_kernel<SDF_FLOW_LOSS_BF16>, grid, dim3(kFlThreads), 0, s, L, d->label, d->mask, d->n_valid, d->levels, d->B,
               d->H, d->W, tiles_x, d->flow_scaling, c0, part);
  } else {
    SDF_LAUNCH(flow_loss_partial_kernel<SDF_FLOW_LOSS_F16>, grid, dim3(kFlThreads), 0, s, L, d->label, d->mask, d->n_valid, d->levels, d->B,
               d->H, d->W, tiles_x, d->flow_scaling, c0, part);
  }
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(flow_loss_finish_kernel, dim3(1), dim3(kFlThreads), 0, s, part, (int)tiles, d->levels, d->B, d->n_valid, d->lambda_mod,
             d->records, d->loss);
  SDF_LAUNCH_CHECK();
  return 0;
}
