// GLIF neuron (the reference's GatedLIFNode, `neuron_type: glif`, Spiking_submodules.py:94-181) for gfx950: multi-step forward and
// BPTT backward with the gradient of the derived gate table - the counterpart of neuron.hip / neuron_bwd.hip for the one neuron
// whose spike is not detached between steps.
//
// The gates are layer-wise scalars.  The caller forms the derived table `tab` = [L, Dk, g, R, th, c_0 .. c_{T-1}] (neuron_step.h
// GlifGates) as 5 + T fp32 in DEVICE memory with its own sigmoids on the same stream; the kernels read it from there, the host
// never does, and autograd carries grad_tab on to the 7 + T logits through that small expression.
//
// Same streaming shape as the LIF kernels: a lane owns 4 consecutive neurons and issues all its 16-byte loads up front.  The
// backward recomputes the trajectory u_t in registers from x with the forward's exact arithmetic (the forward saves nothing), walks
// time backwards (glif_bwd_step) and sums the 5 + T table gradients per lane -> wave butterfly -> workgroup (LDS) -> one row of
// partials per workgroup in the caller's workspace -> glif_bwd_finish_kernel, a fixed-shape tree: no atomics, two calls give
// bit-equal results.  Lanes past the end re-read the last quad and add nothing.
#include "common.h"
#include "host_launch.h"
#include "neuron_step.h"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ GlifGates load_gates(const float* tab) {
  GlifGates G;
  G.L = tab[0]; G.Dk = tab[1]; G.g = tab[2]; G.R = tab[3]; G.th = tab[4];
  return G;
}

template <int TT, bool U8>
__global__ __launch_bounds__(256) void glif_fwd_kernel(const float* x, const float* tab, void* spike, int64_t N) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= N) return;
  const int64_t e = q * 4;
  float4 xv[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) xv[t] = ld4(x + (int64_t)t * N + e);
  const GlifGates G = load_gates(tab);
  float v[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float c = tab[5 + t];
    const float xs[4] = {xv[t].x, xv[t].y, xv[t].z, xv[t].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) glif_step(v[j], s[j], xs[j], c, G);
    if constexpr (U8) {
      const uint32_t w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
      *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(spike) + (int64_t)t * N + e) = w;
    } else {
      st4(reinterpret_cast<float*>(spike) + (int64_t)t * N + e, make_float4(s[0], s[1], s[2], s[3]));
    }
  }
}

struct GlifBwdParams {
  const float* x;
  const float* tab;
  const float* gs;
  float* gx;
  float* partial;                  // [nblk][5 + T]
  int64_t N;
  float c_atan, half_alpha;        // (float)(pi/2 * alpha), (float)(alpha/2)
};

// accumulators: 0 dL, 1 dDk, 2 dg, 3 dR, 4 dth, 5 + t dc_t
template <int TT>
__global__ __launch_bounds__(256) void glif_bwd_kernel(GlifBwdParams P) {
  constexpr int NACC = 5 + TT;
  __shared__ float red[4][NACC];
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = q * 4 < P.N;
  const int64_t e = live ? q * 4 : P.N - 4;
  float4 xv[TT], gv[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) xv[t] = ld4(P.x + (int64_t)t * P.N + e);
#pragma unroll
  for (int t = 0; t < TT; ++t) gv[t] = ld4(P.gs + (int64_t)t * P.N + e);
  const GlifGates G = load_gates(P.tab);
  float ux[TT][4];                                             // u_t (= v_t), per step and neuron
  {
    float v[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float c = P.tab[5 + t];
      const float xs[4] = {xv[t].x, xv[t].y, xv[t].z, xv[t].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ux[t][j] = glif_step(v[j], s[j], xs[j], c, G);
    }
  }
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  float gu[4] = {0.f, 0.f, 0.f, 0.f};                          // dL/du_{t+1} (nothing flows back into the last step)
#pragma unroll
  for (int t = TT - 1; t >= 0; --t) {
    const float c = P.tab[5 + t];
    const float xs[4] = {xv[t].x, xv[t].y, xv[t].z, xv[t].w};
    const float gs[4] = {gv[t].x, gv[t].y, gv[t].z, gv[t].w};
    float gx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float u = ux[t][j];
      float sg;
      gu[j] = glif_bwd_step(gu[j], gs[j], u, spike_of(u, G.th), G, P.c_atan, P.half_alpha, sg);
      gx[j] = gu[j] * c;
      acc[1] -= gu[j];
      acc[4] -= sg;
      acc[5 + t] = __builtin_fmaf(gu[j], xs[j], acc[5 + t]);
      if (t > 0) {                                             // v_{-1} = s_{-1} = 0: step 0 has no membrane or reset term
        const float vp = ux[t - 1][j], sp = spike_of(vp, G.th);
        acc[0] = __builtin_fmaf(gu[j], vp - (vp * G.g) * sp, acc[0]);
        acc[2] = __builtin_fmaf(-gu[j], (G.L * vp) * sp, acc[2]);
        acc[3] = __builtin_fmaf(-gu[j], sp, acc[3]);
      }
    }
    if (live) st4(P.gx + (int64_t)t * P.N + e, make_float4(gx[0], gx[1], gx[2], gx[3]));
  }
  if (!live) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  }
  // butterfly over the 64 lanes, step-major: the exchanges of one step are independent and stay in flight together
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    float other[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) other[i] = __shfl_xor(acc[i], o);
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] += other[i];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) red[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < NACC)
    P.partial[(int64_t)blockIdx.x * NACC + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one workgroup per table entry: strided sums of the per-workgroup partials, then a fixed-shape LDS tree - run-to-run bit-equal
__global__ __launch_bounds__(256) void glif_bwd_finish_kernel(const float* partial, int64_t nblk, int nacc, float* grad_tab) {
  __shared__ float sm[256];
  const int i = blockIdx.x;
  float s = 0.f;
  for (int64_t b = threadIdx.x; b < nblk; b += 256) s += partial[b * nacc + i];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad_tab[i] = sm[0];
}
}  // namespace

extern "C" int sdf_glif_fwd(const float* x, const float* tab, void* spike, int T, int64_t N, int spike_dtype, void* stream) {
  if (!x || !tab || !spike) return SDF_E_NULL;
  if (N < 4 || N % 4 || !sdf_in(SDF_T_GLIF, T) || sdf_quad_blocks(N) >= (1LL << 31)) return SDF_E_SHAPE;
  if (spike_dtype != SDF_F32 && spike_dtype != SDF_U8) return SDF_E_DTYPE;
  if (!sdf_aligned(x, 16) || !sdf_aligned(spike, spike_dtype == SDF_F32 ? 16 : 4) || !sdf_aligned(tab, 4)) return SDF_E_ALIGN;
  dim3 grid((unsigned)sdf_quad_blocks(N)), block(256);
  hipStream_t s = sdf_stream(stream);
  if (!sdf_dispatch(SDF_T_GLIF, T, [&](auto tt) {
        if (spike_dtype == SDF_U8) SDF_LAUNCH((glif_fwd_kernel<tt, true>), grid, block, 0, s, x, tab, spike, N);
        else SDF_LAUNCH((glif_fwd_kernel<tt, false>), grid, block, 0, s, x, tab, spike, N);
      }))
    return SDF_E_SHAPE;
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t sdf_glif_bwd_workspace_bytes(int T, int64_t N) {
  if (!sdf_in(SDF_T_GLIF, T) || N < 4) return 0;
  return sdf_quad_blocks(N) * (5 + T) * (int64_t)sizeof(float);      // one row of 5 + T fp32 partials per workgroup
}

extern "C" int sdf_glif_bwd(const float* x, const float* tab, const float* grad_spike, float* grad_x, float* grad_tab,
                            void* workspace, int64_t workspace_bytes, int T, int64_t N, int surrogate, float alpha, void* stream) {
  if (!x || !tab || !grad_spike || !grad_x || !grad_tab || !workspace) return SDF_E_NULL;
  if (N < 4 || N % 4 || !sdf_in(SDF_T_GLIF, T) || sdf_quad_blocks(N) >= (1LL << 31)) return SDF_E_SHAPE;
  if (surrogate != SDF_SURROGATE_ATAN) return SDF_E_SHAPE;        // ATan is the only surrogate built
  if (workspace_bytes < sdf_glif_bwd_workspace_bytes(T, N)) return SDF_E_SHAPE;
  if (!sdf_aligned(x, 16) || !sdf_aligned(grad_spike, 16) || !sdf_aligned(grad_x, 16) || !sdf_aligned(tab, 4) ||
      !sdf_aligned(grad_tab, 4) || !sdf_aligned(workspace, 4))
    return SDF_E_ALIGN;
  GlifBwdParams P = {};
  P.x = x; P.tab = tab; P.gs = grad_spike; P.gx = grad_x; P.partial = reinterpret_cast<float*>(workspace); P.N = N;
  sdf_atan_consts(alpha, P.c_atan, P.half_alpha);
  const int64_t nblk = sdf_quad_blocks(N);
  dim3 grid((unsigned)nblk), block(256);
  hipStream_t s = sdf_stream(stream);
  if (!sdf_dispatch(SDF_T_GLIF, T, [&](auto tt) { SDF_LAUNCH(glif_bwd_kernel<tt>, grid, block, 0, s, P); })) return SDF_E_SHAPE;
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(glif_bwd_finish_kernel, dim3(5 + T), dim3(256), 0, s, P.partial, nblk, 5 + T, grad_tab);
  SDF_LAUNCH_CHECK();
  return 0;
}
