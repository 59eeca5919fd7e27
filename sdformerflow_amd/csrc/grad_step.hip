// The tail of a training step on flat fp32 gradient buckets, gfx950: per-parameter gradient statistics, the clip coefficient and the
// AdamW update (include/sdformerflow_hip.h: sdf_grad_stats_fwd, sdf_grad_clip_coef, sdf_adamw_step) - and the same tail under a loss
// scaler, with skipped steps and gradient accumulation (sdf_grad_scale_inplace, sdf_grad_clip_scale_coef, sdf_adamw_step_scaled): a
// device-resident SdfLossScaleState carries the verdict on a step and the factor to divide out, and the update obeys it unasked.
//
// Replaces what train.train_step ran in stock torch behind loss.backward(): clip_grad_norm_'s multi-tensor norm and scale passes,
// optimizer.step()'s multi-tensor passes over parameters, gradients and moments, and - for `vis.store_grads` - the reference's three
// .item() read-backs per weight (utils/gradients.py).  One pass over a bucket gives every parameter's sum |g|, sum g^2, min |g|,
// max |g| and non-finite count; that pass feeds both the stored record and the global norm.  A second pass is the clipped update and
// reads the coefficient from device memory: nothing waits for the host.
//
// A parameter is a segment [offset, offset + length) of the flat buffer, packed at any element offset (a length-1 PLIF w shifts all
// that follow).  Both streaming kernels share one geometry: workgroup (x, s) of a (kGsGroups, nseg) grid walks the 16-byte vectors
// between segment s's first and last 16-byte boundary in chunks x, x + kGsGroups, ...; workgroup (0, s) also takes the up to 3 floats
// in front and behind, one lane each.  Fixed chunks, no atomics: the statistics' partial records are combined by a second kernel in a
// fixed order, so two runs on the same bytes give the same bytes.  Compiled with -ffp-contract=off: every fp32 operation of the
// update is rounded on its own, in torch.optim.AdamW(foreach=False)'s order.
//
// Launch sequences: statistics: partial records (kGsGroups x nseg) | finish (nseg).  coefficient (with or without the scaler): one
// workgroup.  update, in-place scale: (kGsGroups x nseg).
#include "host_launch.h"

namespace {

constexpr int kGsThreads = 256;
constexpr int kGsGroups = 128;                           // workgroups (= partial records) per segment
constexpr int kGsFields = 5;                             // sum_abs, sum_sq, min_abs, max_abs, nonfinite
constexpr int kGsVecs = 4;                               // statistics: 16-byte loads per lane and chunk (a chunk is 16 KiB)
constexpr int kAwVecs = 2;                               // update: vectors per lane and chunk (4 streams: 8 loads in flight)
constexpr int64_t kGsMaxFloats = 1ll << 40;

// where the 16-byte vectors of a segment lie
struct GsSpan {
  int64_t head, nvec, tail0;                             // floats in front of the first boundary, whole vectors, first float behind them
};

__device__ __forceinline__ GsSpan gs_span(const float* base, int64_t len) {
  GsSpan S;
  S.head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(base) & 15)) & 15) >> 2);
  if (S.head > len) S.head = len;
  S.nvec = (len - S.head) >> 2;
  S.tail0 = S.head + (S.nvec << 2);
  return S;
}

struct GsAcc {
  double sabs = 0.0, ssq = 0.0, mn = __builtin_inf(), mx = 0.0;
  unsigned long long bad = 0;
};

__device__ __forceinline__ void gs_take(GsAcc& A, float g) {
  const double a = (double)fabsf(g);
  if (!(a < __builtin_inf())) {                          // inf, -inf, NaN
    ++A.bad;
    return;
  }
  A.sabs += a;
  A.ssq += a * a;
  A.mn = a < A.mn ? a : A.mn;
  A.mx = a > A.mx ? a : A.mx;
}

__device__ __forceinline__ void gs_merge(GsAcc& A, double sabs, double ssq, double mn, double mx, unsigned long long bad) {
  A.sabs += sabs;
  A.ssq += ssq;
  A.mn = mn < A.mn ? mn : A.mn;
  A.mx = mx > A.mx ? mx : A.mx;
  A.bad += bad;
}

__device__ __forceinline__ void gs_wave_reduce(GsAcc& A) {
  for (int off = 32; off > 0; off >>= 1)
    gs_merge(A, __shfl_xor(A.sabs, off), __shfl_xor(A.ssq, off), __shfl_xor(A.mn, off), __shfl_xor(A.mx, off),
             (unsigned long long)__shfl_xor((long long)A.bad, off));
}

// workgroup (x, s): one partial record of segment s at part + (s * kGsGroups + x) * kGsFields
__global__ __launch_bounds__(kGsThreads) void grad_stats_partial_kernel(const float* __restrict__ flat, const int64_t* __restrict__ seg,
                                                                        double* __restrict__ part) {
  const int s = blockIdx.y, x = blockIdx.x;
  const int64_t len = seg[2 * s + 1];
  const float* base = flat + seg[2 * s];
  const GsSpan S = gs_span(base, len);
  const float4* body = reinterpret_cast<const float4*>(base + S.head);
  GsAcc A;
  for (int64_t v0 = (int64_t)x * (kGsThreads * kGsVecs); v0 < S.nvec; v0 += (int64_t)kGsGroups * (kGsThreads * kGsVecs)) {
    float4 w[kGsVecs];
#pragma unroll
    for (int k = 0; k < kGsVecs; ++k) {                  // every load of the chunk is issued before the first use
      const int64_t i = v0 + k * kGsThreads + threadIdx.x;
      w[k] = i < S.nvec ? body[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kGsVecs; ++k) {
      if (v0 + k * kGsThreads + threadIdx.x < S.nvec) {
        gs_take(A, w[k].x);
        gs_take(A, w[k].y);
        gs_take(A, w[k].z);
        gs_take(A, w[k].w);
      }
    }
  }
  if (x == 0) {                                          // lanes 0 .. 2: the head floats, lanes 16 .. 18: the tail floats
    const int64_t i = threadIdx.x;
    if (i < S.head)
      gs_take(A, base[i]);
    else if (i >= 16 && i < 19 && S.tail0 + (i - 16) < len)
      gs_take(A, base[S.tail0 + (i - 16)]);
  }
  gs_wave_reduce(A);
  constexpr int W = kGsThreads / 64;
  __shared__ double r_d[W][4];
  __shared__ unsigned long long r_bad[W];
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    r_d[w][0] = A.sabs; r_d[w][1] = A.ssq; r_d[w][2] = A.mn; r_d[w][3] = A.mx;
    r_bad[w] = A.bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    GsAcc T;
    for (int w = 0; w < W; ++w) gs_merge(T, r_d[w][0], r_d[w][1], r_d[w][2], r_d[w][3], r_bad[w]);
    double* p = part + ((int64_t)s * kGsGroups + x) * kGsFields;
    p[0] = T.sabs; p[1] = T.ssq; p[2] = T.mn; p[3] = T.mx; p[4] = (double)T.bad;
  }
}

// segment blockIdx.x: lane l takes partials l and l + 64, then the wave's fixed exchange tree; lane 0 writes the row
__global__ __launch_bounds__(64) void grad_stats_finish_kernel(const double* __restrict__ part, double* __restrict__ rows) {
  static_assert(kGsGroups == 128, "two partial records per lane");
  const int s = blockIdx.x, l = threadIdx.x;
  const double* p = part + ((int64_t)s * kGsGroups + l) * kGsFields;
  const double* q = p + 64 * kGsFields;
  GsAcc A;
  gs_merge(A, p[0], p[1], p[2], p[3], (unsigned long long)p[4]);
  gs_merge(A, q[0], q[1], q[2], q[3], (unsigned long long)q[4]);
  gs_wave_reduce(A);
  if (l == 0) {
    double* r = rows + (int64_t)s * kGsFields;
    r[0] = A.sabs; r[1] = A.ssq; r[2] = A.mn; r[3] = A.mx; r[4] = (double)A.bad;
  }
}

// one workgroup: lane t adds rows t, t + 256, ... in row order, then wave tree, then the 4 waves in order.  True on thread 0 alone,
// which then holds the sum of squares `s` and the non-finite count `b` of the masked rows.
__device__ __forceinline__ bool gc_reduce(const double* __restrict__ table, int rows, const uint8_t* __restrict__ mask, double& s, double& b) {
  double ssq = 0.0, bad = 0.0;
  for (int r = threadIdx.x; r < rows; r += kGsThreads) {
    if (mask && !mask[r]) continue;
    ssq += table[(int64_t)r * kGsFields + 1];
    bad += table[(int64_t)r * kGsFields + 4];
  }
  for (int off = 32; off > 0; off >>= 1) {
    ssq += __shfl_xor(ssq, off);
    bad += __shfl_xor(bad, off);
  }
  constexpr int W = kGsThreads / 64;
  __shared__ double r_s[W], r_b[W];
  if ((threadIdx.x & 63) == 0) {
    r_s[threadIdx.x >> 6] = ssq;
    r_b[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  s = 0.0;
  b = 0.0;
  for (int w = 0; w < W; ++w) {
    s += r_s[w];
    b += r_b[w];
  }
  return true;
}

__global__ __launch_bounds__(kGsThreads) void grad_clip_coef_kernel(const double* __restrict__ table, int rows, const uint8_t* __restrict__ mask,
                                                                    double max_norm, float* __restrict__ coef, double* __restrict__ record) {
  double s, b;
  if (gc_reduce(table, rows, mask, s, b)) {
    const double total = sqrt(s);
    const double c = max_norm / (total + 1e-6);
    record[0] = total;
    record[1] = b;
    coef[0] = (float)(c < 1.0 ? c : 1.0);
  }
}

// ... and the loss scaler behind the same reduction: the verdict on this step, the reciprocal of the scale its gradients carry, and
// then torch's _amp_update_scale_ for the next one
__global__ __launch_bounds__(kGsThreads) void grad_clip_scale_coef_kernel(const double* __restrict__ table, int rows,
                                                                          const uint8_t* __restrict__ mask, double max_norm,
                                                                          float* __restrict__ coef, double* __restrict__ record,
                                                                          SdfLossScaleState* __restrict__ state, float growth, float backoff,
                                                                          int growth_interval, int clip_unscaled, int update) {
  double s, b;
  if (gc_reduce(table, rows, mask, s, b)) {
    const double total = sqrt(s);
    const float scale = state->scale;
    const float inv = (float)(1.0 / (double)scale);
    const double c = max_norm / ((clip_unscaled ? total * (double)inv : total) + 1e-6);
    record[0] = total;
    record[1] = b;
    coef[0] = (float)(c < 1.0 ? c : 1.0);
    const int found = b > 0.0 ? 1 : 0;
    state->found_inf = found;
    state->inv_scale = inv;
    state->skipped += found;
    if (update) {
      if (found) {
        state->scale = scale * backoff;
        state->growth_tracker = 0;
      } else if (state->growth_tracker + 1 == growth_interval) {
        const float grown = scale * growth;
        if (fabsf(grown) < __builtin_inff()) state->scale = grown;
        state->growth_tracker = 0;
      } else {
        state->growth_tracker += 1;
      }
    }
  }
}

struct AwScalars {
  float decay, w1, beta2, w2, nstep, bc2s, eps, c, inv;
};

// kScaled: the gradient carries a loss scale - a second multiplication, by its reciprocal, behind the clip's
template <bool kScaled>
__device__ __forceinline__ void aw_elem(const AwScalars& S, float g, float& m, float& v, float& p) {
  g = g * S.c;
  if (kScaled) g = g * S.inv;
  p = p * S.decay;
  const float diff = g - m;
  m = S.w1 < 0.5f ? m + S.w1 * diff : g - diff * (1.0f - S.w1);
  v = v * S.beta2;
  v = v + (S.w2 * g) * g;
  const float denom = sqrtf(v) / S.bc2s + S.eps;
  p = p + (S.nstep * m) / denom;
}

// the update of segment blockIdx.y by workgroup blockIdx.x, shared by the two kernels below.  kScaled: `state` decides - a step with a
// non-finite gradient writes nothing at all, any other one divides the scale out
template <bool kScaled>
__device__ __forceinline__ void aw_segment(const float* __restrict__ grad, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                           const SdfAdamwRow* __restrict__ rows, const float* __restrict__ coef,
                                           const SdfLossScaleState* __restrict__ state) {
  const SdfAdamwRow R = rows[blockIdx.y];
  if (!R.active) return;
  const int x = blockIdx.x;
  AwScalars S;
  S.decay = R.decay; S.w1 = R.w1; S.beta2 = R.beta2; S.w2 = R.w2; S.nstep = R.neg_step_size; S.bc2s = R.bc2_sqrt; S.eps = R.eps;
  S.c = coef ? coef[0] : 1.0f;
  S.inv = 1.0f;
  if (kScaled) {
    if (state->found_inf != 0) return;
    S.inv = state->inv_scale;
  }
  const float* g = grad + R.offset;
  float* m = exp_avg + R.offset;
  float* v = exp_avg_sq + R.offset;
  float* p = static_cast<float*>(R.param);
  const GsSpan G = gs_span(g, R.length);                 // (the three flat buffers share their position within 16 bytes: one span serves them)
  const bool pvec = ((reinterpret_cast<uintptr_t>(p + G.head)) & 15) == 0;
  const float4* g4 = reinterpret_cast<const float4*>(g + G.head);
  float4* m4 = reinterpret_cast<float4*>(m + G.head);
  float4* v4 = reinterpret_cast<float4*>(v + G.head);
  float* pb = p + G.head;
  for (int64_t v0 = (int64_t)x * (kGsThreads * kAwVecs); v0 < G.nvec; v0 += (int64_t)kGsGroups * (kGsThreads * kAwVecs)) {
    float4 gw[kAwVecs], mw[kAwVecs], vw[kAwVecs], pw[kAwVecs];
#pragma unroll
    for (int k = 0; k < kAwVecs; ++k) {
      const int64_t i = v0 + k * kGsThreads + threadIdx.x;
      if (i < G.nvec) {
        gw[k] = g4[i];
        mw[k] = m4[i];
        vw[k] = v4[i];
        if (pvec) {
          pw[k] = reinterpret_cast<const float4*>(pb)[i];
        } else {
          pw[k].x = pb[4 * i]; pw[k].y = pb[4 * i + 1]; pw[k].z = pb[4 * i + 2]; pw[k].w = pb[4 * i + 3];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kAwVecs; ++k) {
      const int64_t i = v0 + k * kGsThreads + threadIdx.x;
      if (i < G.nvec) {
        aw_elem<kScaled>(S, gw[k].x, mw[k].x, vw[k].x, pw[k].x);
        aw_elem<kScaled>(S, gw[k].y, mw[k].y, vw[k].y, pw[k].y);
        aw_elem<kScaled>(S, gw[k].z, mw[k].z, vw[k].z, pw[k].z);
        aw_elem<kScaled>(S, gw[k].w, mw[k].w, vw[k].w, pw[k].w);
        m4[i] = mw[k];
        v4[i] = vw[k];
        if (pvec) {
          reinterpret_cast<float4*>(pb)[i] = pw[k];
        } else {
          pb[4 * i] = pw[k].x; pb[4 * i + 1] = pw[k].y; pb[4 * i + 2] = pw[k].z; pb[4 * i + 3] = pw[k].w;
        }
      }
    }
  }
  if (x == 0) {                                          // lanes 0 .. 2: the head floats, lanes 16 .. 18: the tail floats
    int64_t i = threadIdx.x;
    bool mine = i < G.head;
    if (!mine && i >= 16 && i < 19 && G.tail0 + (i - 16) < R.length) {
      i = G.tail0 + (i - 16);
      mine = true;
    }
    if (mine) {
      float mm = m[i], vv = v[i], pp = p[i];
      aw_elem<kScaled>(S, g[i], mm, vv, pp);
      m[i] = mm;
      v[i] = vv;
      p[i] = pp;
    }
  }
}

__global__ __launch_bounds__(kGsThreads) void adamw_step_kernel(const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                float* __restrict__ exp_avg_sq, const SdfAdamwRow* __restrict__ rows,
                                                                const float* __restrict__ coef) {
  aw_segment<false>(grad, exp_avg, exp_avg_sq, rows, coef, nullptr);
}

__global__ __launch_bounds__(kGsThreads) void adamw_step_scaled_kernel(const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                       float* __restrict__ exp_avg_sq, const SdfAdamwRow* __restrict__ rows,
                                                                       const float* __restrict__ coef,
                                                                       const SdfLossScaleState* __restrict__ state) {
  aw_segment<true>(grad, exp_avg, exp_avg_sq, rows, coef, state);
}

// g *= coef[0] over the active segments: workgroup (x, s) of a (kGsGroups, nseg) grid, the statistics kernel's chunks
__global__ __launch_bounds__(kGsThreads) void grad_scale_kernel(float* __restrict__ flat, const int64_t* __restrict__ seg,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ coef) {
  const int s = blockIdx.y, x = blockIdx.x;
  if (mask && !mask[s]) return;
  const float c = coef[0];
  const int64_t len = seg[2 * s + 1];
  float* base = flat + seg[2 * s];
  const GsSpan S = gs_span(base, len);
  float4* body = reinterpret_cast<float4*>(base + S.head);
  for (int64_t v0 = (int64_t)x * (kGsThreads * kGsVecs); v0 < S.nvec; v0 += (int64_t)kGsGroups * (kGsThreads * kGsVecs)) {
    float4 w[kGsVecs];
#pragma unroll
    for (int k = 0; k < kGsVecs; ++k) {                  // every load of the chunk is issued before the first store
      const int64_t i = v0 + k * kGsThreads + threadIdx.x;
      if (i < S.nvec) w[k] = body[i];
    }
#pragma unroll
    for (int k = 0; k < kGsVecs; ++k) {
      const int64_t i = v0 + k * kGsThreads + threadIdx.x;
      if (i < S.nvec) {
        w[k].x = w[k].x * c; w[k].y = w[k].y * c; w[k].z = w[k].z * c; w[k].w = w[k].w * c;
        body[i] = w[k];
      }
    }
  }
  if (x == 0) {                                          // lanes 0 .. 2: the head floats, lanes 16 .. 18: the tail floats
    const int64_t i = threadIdx.x;
    if (i < S.head)
      base[i] = base[i] * c;
    else if (i >= 16 && i < 19 && S.tail0 + (i - 16) < len)
      base[S.tail0 + (i - 16)] = base[S.tail0 + (i - 16)] * c;
  }
}

// segments ascend, do not overlap and lie inside [0, n): `at(i, off, len)` reads row i of the host table
template <class F>
inline bool gs_segments_ok(int nseg, int64_t n, F&& at) {
  int64_t end = 0;
  for (int i = 0; i < nseg; ++i) {
    int64_t off, len;
    at(i, off, len);
    if (off < end || len < 1 || len > n || off > n - len) return false;
    end = off + len;
  }
  return true;
}

// two buffers with one layout whose 16-byte boundaries fall on the same elements
inline bool gs_same_phase(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

inline bool gs_count_ok(int nseg, int64_t n) { return nseg >= 1 && nseg <= 65535 && n >= 1 && n <= kGsMaxFloats; }

}  // namespace

extern "C" int64_t sdf_grad_stats_workspace_bytes(int nseg) {
  return nseg >= 1 && nseg <= 65535 ? (int64_t)nseg * kGsGroups * kGsFields * 8 : 0;
}

extern "C" int sdf_grad_stats_fwd(const SdfGradStatsDesc* d, void* stream) {
  if (!d || !d->flat || !d->seg_host || !d->seg || !d->table || !d->workspace) return SDF_E_NULL;
  if (!gs_count_ok(d->nseg, d->n)) return SDF_E_SHAPE;
  if (!gs_segments_ok(d->nseg, d->n, [&](int i, int64_t& off, int64_t& len) { off = d->seg_host[2 * i]; len = d->seg_host[2 * i + 1]; }))
    return SDF_E_SHAPE;
  if (d->row0 < 0 || (int64_t)d->row0 + d->nseg > d->rows) return SDF_E_SHAPE;     // the records lie inside the table
  if (d->workspace_bytes < sdf_grad_stats_workspace_bytes(d->nseg)) return SDF_E_SHAPE;
  if (!sdf_aligned(d->flat, 4) || !sdf_aligned(d->seg, 8) || !sdf_aligned(d->table, 8) || !sdf_aligned(d->workspace, 8)) return SDF_E_ALIGN;
  if (!sdf_on_device(d->flat) || !sdf_on_device(d->seg) || !sdf_on_device(d->table) || !sdf_on_device(d->workspace)) return SDF_E_DTYPE;
  hipStream_t s = sdf_stream(stream);
  double* part = static_cast<double*>(d->workspace);
  SDF_LAUNCH(grad_stats_partial_kernel, dim3(kGsGroups, d->nseg), dim3(kGsThreads), 0, s, d->flat, d->seg, part);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(grad_stats_finish_kernel, dim3(d->nseg), dim3(64), 0, s, part, d->table + (int64_t)d->row0 * kGsFields);
  return sdf_launch_rc();
}

extern "C" int sdf_grad_clip_coef(const double* table, int rows, const uint8_t* mask, float max_norm, float* coef, double* record,
                                  void* stream) {
  if (!table || !coef || !record) return SDF_E_NULL;
  if (rows < 1 || rows > (1 << 24) || !(max_norm >= 0.f)) return SDF_E_SHAPE;                  // (+inf: no clip, coef 1)
  if (!sdf_aligned(table, 8) || !sdf_aligned(record, 8) || !sdf_aligned(coef, 4)) return SDF_E_ALIGN;
  if (!sdf_on_device(table) || (mask && !sdf_on_device(mask)) || !sdf_on_device(coef) || !sdf_on_device(record)) return SDF_E_DTYPE;
  SDF_LAUNCH(grad_clip_coef_kernel, dim3(1), dim3(kGsThreads), 0, sdf_stream(stream), table, rows, mask, (double)max_norm, coef, record);
  return sdf_launch_rc();
}

namespace {

// the checks of sdf_adamw_step and of its scaled form (`scaled`: with a loss-scale state), in the family's order: 0, or the refusal
inline int aw_check(const SdfAdamwDesc* d, const SdfLossScaleState* state, bool scaled) {
  if (scaled && !state) return SDF_E_NULL;
  if (!d || !d->grad || !d->exp_avg || !d->exp_avg_sq || !d->rows_host || !d->rows) return SDF_E_NULL;
  if (!gs_count_ok(d->nseg, d->n)) return SDF_E_SHAPE;
  for (int i = 0; i < d->nseg; ++i)
    if (d->rows_host[i].active && !d->rows_host[i].param) return SDF_E_NULL;
  if (!gs_segments_ok(d->nseg, d->n, [&](int i, int64_t& off, int64_t& len) { off = d->rows_host[i].offset; len = d->rows_host[i].length; }))
    return SDF_E_SHAPE;
  if (!sdf_aligned(d->grad, 4) || !sdf_aligned(d->rows, 8) || !sdf_aligned(d->coef, 4)) return SDF_E_ALIGN;
  if (scaled && !sdf_aligned(state, 8)) return SDF_E_ALIGN;
  if (!gs_same_phase(d->grad, d->exp_avg) || !gs_same_phase(d->grad, d->exp_avg_sq)) return SDF_E_ALIGN;
  for (int i = 0; i < d->nseg; ++i)
    if (d->rows_host[i].active && !sdf_aligned(d->rows_host[i].param, 4)) return SDF_E_ALIGN;
  if (!sdf_on_device(d->grad) || !sdf_on_device(d->exp_avg) || !sdf_on_device(d->exp_avg_sq) || !sdf_on_device(d->rows) ||
      (d->coef && !sdf_on_device(d->coef)) || (scaled && !sdf_on_device(state)))
    return SDF_E_DTYPE;
  for (int i = 0; i < d->nseg; ++i)
    if (d->rows_host[i].active && !sdf_on_device(d->rows_host[i].param)) return SDF_E_DTYPE;
  return 0;
}

}  // namespace

extern "C" int sdf_adamw_step(const SdfAdamwDesc* d, void* stream) {
  if (const int rc = aw_check(d, nullptr, false)) return rc;
  SDF_LAUNCH(adamw_step_kernel, dim3(kGsGroups, d->nseg), dim3(kGsThreads), 0, sdf_stream(stream), d->grad, d->exp_avg, d->exp_avg_sq, d->rows,
             d->coef);
  return sdf_launch_rc();
}

extern "C" int sdf_adamw_step_scaled(const SdfAdamwDesc* d, const SdfLossScaleState* state, void* stream) {
  if (const int rc = aw_check(d, state, true)) return rc;
  SDF_LAUNCH(adamw_step_scaled_kernel, dim3(kGsGroups, d->nseg), dim3(kGsThreads), 0, sdf_stream(stream), d->grad, d->exp_avg, d->exp_avg_sq,
             d->rows, d->coef, state);
  return sdf_launch_rc();
}

extern "C" int sdf_grad_scale_inplace(const SdfGradScaleDesc* d, void* stream) {
  if (!d || !d->flat || !d->seg_host || !d->seg || !d->coef) return SDF_E_NULL;
  if (!gs_count_ok(d->nseg, d->n)) return SDF_E_SHAPE;
  if (!gs_segments_ok(d->nseg, d->n, [&](int i, int64_t& off, int64_t& len) { off = d->seg_host[2 * i]; len = d->seg_host[2 * i + 1]; }))
    return SDF_E_SHAPE;
  if (!sdf_aligned(d->flat, 4) || !sdf_aligned(d->seg, 8) || !sdf_aligned(d->coef, 4)) return SDF_E_ALIGN;
  if (!sdf_on_device(d->flat) || !sdf_on_device(d->seg) || (d->mask && !sdf_on_device(d->mask)) || !sdf_on_device(d->coef)) return SDF_E_DTYPE;
  SDF_LAUNCH(grad_scale_kernel, dim3(kGsGroups, d->nseg), dim3(kGsThreads), 0, sdf_stream(stream), d->flat, d->seg, d->mask, d->coef);
  return sdf_launch_rc();
}

extern "C" int sdf_grad_clip_scale_coef(const SdfGradClipScaleDesc* d, void* stream) {
  if (!d || !d->table || !d->coef || !d->record || !d->state) return SDF_E_NULL;
  if (d->rows < 1 || d->rows > (1 << 24) || !(d->max_norm >= 0.f)) return SDF_E_SHAPE;            // (+inf: no clip, coef 1)
  if (!(d->growth_factor > 0.f) || !(d->backoff_factor > 0.f) || d->growth_interval < 1) return SDF_E_SHAPE;
  if (!sdf_aligned(d->table, 8) || !sdf_aligned(d->record, 8) || !sdf_aligned(d->coef, 4) || !sdf_aligned(d->state, 8)) return SDF_E_ALIGN;
  if (!sdf_on_device(d->table) || (d->mask && !sdf_on_device(d->mask)) || !sdf_on_device(d->coef) || !sdf_on_device(d->record) ||
      !sdf_on_device(d->state))
    return SDF_E_DTYPE;
  SDF_LAUNCH(grad_clip_scale_coef_kernel, dim3(1), dim3(kGsThreads), 0, sdf_stream(stream), d->table, (int)d->rows, d->mask,
             (double)d->max_norm, d->coef, d->record, d->state, d->growth_factor, d->backoff_factor, (int)d->growth_interval,
             (int)d->clip_unscaled, (int)d->update);
  return sdf_launch_rc();
}
