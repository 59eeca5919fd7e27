// Spiking-neuron state update kernels (LIF / IF / PSN) for gfx950.
//
// HBM-bound streaming kernels: every lane owns 4 consecutive neurons, issues all T of its 16-byte
// loads before the first use (T <= 20 loads in flight per lane hide HBM latency without LDS), runs
// the charge / fire / reset recurrence in registers and writes each spike once (fp32 or 1 byte).
// The eval-BatchNorm affine, the positional-encoding add and the pad / roll / window-partition
// gather that precede the neuron in the reference are folded into the load.
//
// Numerics contract (checked bit-for-bit against oracle/): every LIF operation is a separately
// rounded IEEE fp32 op - this file is compiled with -ffp-contract=off - and the only fused
// operations are the explicit fmaf() of the BN prologue and of the PSN chain.
#include "common.h"
#include "host_launch.h"
#include "neuron_step.h"

namespace {

struct NeuronParams {
  SdfNeuronDesc d;
  int64_t quads;     // nb*ni/4
  int64_t rows;      // gather mode: nb*ni/rowlen
  float inv_tau;     // exact reciprocal when tau is a power of two, else 0
};

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <int KIND>
struct Step;  // charge/fire/reset of one time step on a 4-vector

__device__ __forceinline__ void store_spikes(const NeuronParams& P, int64_t ooff, float4 s) {
  if (P.d.out_dtype == SDF_F32) {
    *reinterpret_cast<float4*>(reinterpret_cast<float*>(P.d.out) + ooff) = s;
  } else {
    uint32_t w = (uint32_t)(s.x != 0.f) | ((uint32_t)(s.y != 0.f) << 8) | ((uint32_t)(s.z != 0.f) << 16) |
                 ((uint32_t)(s.w != 0.f) << 24);
    *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(P.d.out) + ooff) = w;
  }
}

// Address of the quad in x for step t, or nullptr for a padding row.
__device__ __forceinline__ const float* x_addr(const NeuronParams& P, int t, int64_t e, int64_t b, int64_t r, int64_t xrep = 0) {
  if (P.d.rowmap == nullptr) return P.d.x + xrep + b * P.d.x_sb + (int64_t)t * P.d.x_st + r;
  int64_t row = e / P.d.rowlen;
  int64_t col = e - row * P.d.rowlen;
  int32_t src = P.d.rowmap[(int64_t)t * P.rows + row];
  return src < 0 ? nullptr : P.d.x + (int64_t)src * P.d.rowlen + col;
}

__device__ __forceinline__ float4 prologue(const NeuronParams& P, float4 x, int t, int64_t r, float4 al, float4 be) {
  if (P.d.alpha) {
    x.x = __builtin_fmaf(x.x, al.x, be.x);
    x.y = __builtin_fmaf(x.y, al.y, be.y);
    x.z = __builtin_fmaf(x.z, al.z, be.z);
    x.w = __builtin_fmaf(x.w, al.w, be.w);
  }
  if (P.d.add) {
    float4 a = load4(P.d.add + (int64_t)t * P.d.add_st + (r % P.d.add_period));
    x.x += a.x; x.y += a.y; x.z += a.z; x.w += a.w;
  }
  return x;
}

// Where quad q of a launch lies: element e of its problem (batch element b, offset r), the problem's offset in x, the quad's offset
// in out at step 0, and the BN affine of its four channels.
struct Quad {
  int64_t e, xrep, b, r, obase;
  float4 al, be;
};

__device__ __forceinline__ Quad quad_of(const NeuronParams& P, int64_t q) {
  Quad Q;
  int64_t e = q * 4, xrep = 0, orep = 0;
  if (P.d.nrep > 1) {                                            // outermost dimension: nrep equally laid out problems (dense mode)
    const int64_t per = P.d.nb * P.d.ni, rp = e / per;
    e -= rp * per;
    xrep = rp * P.d.x_srep;
    orep = rp * P.d.o_srep;
  }
  const int64_t b = e / P.d.ni;
  const int64_t r = e - b * P.d.ni;
  Q.e = e; Q.xrep = xrep; Q.b = b; Q.r = r;
  Q.obase = orep + b * P.d.o_sb + r;
  Q.al = make_float4(1.f, 1.f, 1.f, 1.f);
  Q.be = make_float4(0.f, 0.f, 0.f, 0.f);
  if (P.d.alpha) {
    if (P.d.inner == 1) {
      int c = (int)(r % P.d.C);
      Q.al = load4(P.d.alpha + c);
      Q.be = load4(P.d.beta + c);
    } else {
      int c = (int)((r / P.d.inner) % P.d.C);
      float a = P.d.alpha[c], bb = P.d.beta[c];
      Q.al = make_float4(a, a, a, a);
      Q.be = make_float4(bb, bb, bb, bb);
    }
  }
  return Q;
}

// T is a compile-time constant (register-resident x) when TT > 0, else runtime (streaming, LIF/IF only).
template <int TT>
__device__ __forceinline__ void neuron_body(const NeuronParams& P, int64_t q) {
  if (q >= P.quads) return;
  const int T = TT > 0 ? TT : P.d.T;
  const Quad Q = quad_of(P, q);
  const int64_t e = Q.e, xrep = Q.xrep, b = Q.b, r = Q.r, obase = Q.obase;
  const float4 al = Q.al, be = Q.be;

  if constexpr (TT > 0) {
    float4 xv[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const float* p = x_addr(P, t, e, b, r, xrep);
      xv[t] = p ? load4(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) xv[t] = prologue(P, xv[t], t, r, al, be);

    if (P.d.kind == SDF_PSN) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float bt = P.d.psn_b[t];
        float4 h = make_float4(bt, bt, bt, bt);
#pragma unroll
        for (int k = 0; k < TT; ++k) {
          const float w = P.d.psn_w[t * TT + k];
          h.x = __builtin_fmaf(w, xv[k].x, h.x);
          h.y = __builtin_fmaf(w, xv[k].y, h.y);
          h.z = __builtin_fmaf(w, xv[k].z, h.z);
          h.w = __builtin_fmaf(w, xv[k].w, h.w);
        }
        float4 s = make_float4(h.x >= 0.f ? 1.f : 0.f, h.y >= 0.f ? 1.f : 0.f, h.z >= 0.f ? 1.f : 0.f,
                               h.w >= 0.f ? 1.f : 0.f);
        store_spikes(P, obase + (int64_t)t * P.d.o_st, s);
      }
      return;
    }
    const bool soft = P.d.soft_reset != 0;
    const bool reset0 = soft || P.d.v_reset == 0.f, is_if = P.d.kind == SDF_IF;
    const float v0 = soft ? 0.f : P.d.v_reset;
    float4 v = make_float4(v0, v0, v0, v0);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float4 h, s;
      h.x = neuron_charge(is_if, v.x, xv[t].x, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.y = neuron_charge(is_if, v.y, xv[t].y, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.z = neuron_charge(is_if, v.z, xv[t].z, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.w = neuron_charge(is_if, v.w, xv[t].w, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      s.x = fire_reset(v.x, h.x, P.d.v_th, P.d.v_reset, soft);
      s.y = fire_reset(v.y, h.y, P.d.v_th, P.d.v_reset, soft);
      s.z = fire_reset(v.z, h.z, P.d.v_th, P.d.v_reset, soft);
      s.w = fire_reset(v.w, h.w, P.d.v_th, P.d.v_reset, soft);
      store_spikes(P, obase + (int64_t)t * P.d.o_st, s);
    }
    if (P.d.v_last) *reinterpret_cast<float4*>(P.d.v_last + q * 4) = v;
  } else {
    // runtime T: sequential neurons only (PSN with an unlisted T is rejected on the host)
    const bool soft = P.d.soft_reset != 0;
    const bool reset0 = soft || P.d.v_reset == 0.f, is_if = P.d.kind == SDF_IF;
    const float v0 = soft ? 0.f : P.d.v_reset;
    float4 v = make_float4(v0, v0, v0, v0);
    const float* p = x_addr(P, 0, e, b, r, xrep);
    float4 nxt = p ? load4(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < T; ++t) {
      float4 x = nxt;
      if (t + 1 < T) {
        const float* pn = x_addr(P, t + 1, e, b, r, xrep);
        nxt = pn ? load4(pn) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      x = prologue(P, x, t, r, al, be);
      float4 h, s;
      h.x = neuron_charge(is_if, v.x, x.x, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.y = neuron_charge(is_if, v.y, x.y, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.z = neuron_charge(is_if, v.z, x.z, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      h.w = neuron_charge(is_if, v.w, x.w, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
      s.x = fire_reset(v.x, h.x, P.d.v_th, P.d.v_reset, soft);
      s.y = fire_reset(v.y, h.y, P.d.v_th, P.d.v_reset, soft);
      s.z = fire_reset(v.z, h.z, P.d.v_th, P.d.v_reset, soft);
      s.w = fire_reset(v.w, h.w, P.d.v_th, P.d.v_reset, soft);
      store_spikes(P, obase + (int64_t)t * P.d.o_st, s);
    }
    if (P.d.v_last) *reinterpret_cast<float4*>(P.d.v_last + q * 4) = v;
  }
}

template <int TT>
__global__ __launch_bounds__(256) void neuron_kernel(NeuronParams P) {
  neuron_body<TT>(P, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// GLIF (neuron_step.h glif_step, from v = 0, s = 0) behind the same addressing, prologue and spike store: a kernel of its own, so
// that neuron_body keeps its registers.  `tab` = [L, Dk, g, R, th, c_0 .. c_{T-1}] in device memory, as glif.hip takes it.
template <int TT>
__global__ __launch_bounds__(256) void glif_neuron_kernel(NeuronParams P, const float* __restrict__ tab) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= P.quads) return;
  const Quad Q = quad_of(P, q);
  float4 xv[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float* p = x_addr(P, t, Q.e, Q.b, Q.r, Q.xrep);
    xv[t] = p ? load4(p) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) xv[t] = prologue(P, xv[t], t, Q.r, Q.al, Q.be);
  GlifGates G;
  G.L = tab[0]; G.Dk = tab[1]; G.g = tab[2]; G.R = tab[3]; G.th = tab[4];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f), s = v;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float c = tab[5 + t];
    glif_step(v.x, s.x, xv[t].x, c, G);
    glif_step(v.y, s.y, xv[t].y, c, G);
    glif_step(v.z, s.z, xv[t].z, c, G);
    glif_step(v.w, s.w, xv[t].w, c, G);
    store_spikes(P, Q.obase + (int64_t)t * P.d.o_st, s);
  }
}

// The LIF / IF launch that also keeps the membrane: step t's v after the reset (fire_reset's v - spikingjelly's v_seq under
// store_v_seq) goes to v_seq at the spike's own offset, in fp32 elements.  A kernel of its own, as the GLIF one, so that neuron_body
// keeps its registers; TT == 0 is the runtime-T form (one load ahead).  Same step, same order: the spikes are sdf_neuron_fwd's.
template <int TT>
__global__ __launch_bounds__(256) void neuron_vseq_kernel(NeuronParams P, float* __restrict__ v_seq) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= P.quads) return;
  const int T = TT > 0 ? TT : P.d.T;
  const Quad Q = quad_of(P, q);
  const bool soft = P.d.soft_reset != 0;
  const bool reset0 = soft || P.d.v_reset == 0.f, is_if = P.d.kind == SDF_IF;
  const float v0 = soft ? 0.f : P.d.v_reset;
  float4 v = make_float4(v0, v0, v0, v0);
  auto step = [&](int t, float4 x) {
    float4 h, s;
    h.x = neuron_charge(is_if, v.x, x.x, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
    h.y = neuron_charge(is_if, v.y, x.y, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
    h.z = neuron_charge(is_if, v.z, x.z, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
    h.w = neuron_charge(is_if, v.w, x.w, P.d.tau, P.inv_tau, P.d.v_reset, reset0);
    s.x = fire_reset(v.x, h.x, P.d.v_th, P.d.v_reset, soft);
    s.y = fire_reset(v.y, h.y, P.d.v_th, P.d.v_reset, soft);
    s.z = fire_reset(v.z, h.z, P.d.v_th, P.d.v_reset, soft);
    s.w = fire_reset(v.w, h.w, P.d.v_th, P.d.v_reset, soft);
    const int64_t off = Q.obase + (int64_t)t * P.d.o_st;
    store_spikes(P, off, s);
    *reinterpret_cast<float4*>(v_seq + off) = v;
  };
  auto load = [&](int t) {
    const float* p = x_addr(P, t, Q.e, Q.b, Q.r, Q.xrep);
    return p ? load4(p) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  if constexpr (TT > 0) {
    float4 xv[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) xv[t] = load(t);
#pragma unroll
    for (int t = 0; t < TT; ++t) step(t, prologue(P, xv[t], t, Q.r, Q.al, Q.be));
  } else {
    float4 nxt = load(0);
    for (int t = 0; t < T; ++t) {
      const float4 x = nxt;
      if (t + 1 < T) nxt = load(t + 1);
      step(t, prologue(P, x, t, Q.r, Q.al, Q.be));
    }
  }
  if (P.d.v_last) *reinterpret_cast<float4*>(P.d.v_last + q * 4) = v;
}

// Several independent neuron calls of the same T as ONE launch (the decoders' skip inputs: four small tensors, each a launch of
// its own before): workgroup ranges are dealt to the descriptors by `first[]`
constexpr int MULTI_MAX = 6;
struct NeuronMulti {
  NeuronParams p[MULTI_MAX];
  int first[MULTI_MAX + 1];       // first workgroup of descriptor i; first[n] = grid size
  int n;
};

template <int TT>
__global__ __launch_bounds__(256) void neuron_multi_kernel(NeuronMulti M) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < MULTI_MAX; ++k)
    if (k < M.n && (int)blockIdx.x >= M.first[k]) i = k;
  i = __builtin_amdgcn_readfirstlane(i);
  // (select by a chain of wave-uniform compares: an indexed copy of a by-value struct would live in scratch)
#define SDF_MULTI_CASE(k) if (i == k) { neuron_body<TT>(M.p[k], (int64_t)((int)blockIdx.x - M.first[k]) * 256 + threadIdx.x); return; }
  SDF_MULTI_CASE(0) SDF_MULTI_CASE(1) SDF_MULTI_CASE(2) SDF_MULTI_CASE(3) SDF_MULTI_CASE(4) SDF_MULTI_CASE(5)
#undef SDF_MULTI_CASE
}

// One neuron per lane, any N: the contiguous (T, N) entry points use it when N is not a multiple of 4 (rows of such a
// buffer are not 16-byte aligned, so the streaming kernel's float4 accesses do not apply).  Same op sequence.
__global__ __launch_bounds__(256) void neuron_scalar_kernel(const float* __restrict__ x, void* __restrict__ out, float* __restrict__ v_last,
                                                            int T, int64_t N, int kind, float tau, float inv_tau, float v_th,
                                                            float v_reset, int soft_i, int out_dtype, const float* __restrict__ psn_w,
                                                            const float* __restrict__ psn_b) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const bool soft = soft_i != 0;
  auto put = [&](int t, float sp) {
    if (out_dtype == SDF_F32) reinterpret_cast<float*>(out)[(int64_t)t * N + n] = sp;
    else reinterpret_cast<uint8_t*>(out)[(int64_t)t * N + n] = sp != 0.f ? 1 : 0;
  };
  if (kind == SDF_PSN) {
    for (int t = 0; t < T; ++t) {
      float h = psn_b[t];
      for (int k = 0; k < T; ++k) h = __builtin_fmaf(psn_w[t * T + k], x[(int64_t)k * N + n], h);
      put(t, h >= 0.f ? 1.f : 0.f);
    }
    return;
  }
  const bool reset0 = soft || v_reset == 0.f;
  float v = soft ? 0.f : v_reset;
  for (int t = 0; t < T; ++t) {
    const float xt = x[(int64_t)t * N + n];
    const float h = neuron_charge(kind == SDF_IF, v, xt, tau, inv_tau, v_reset, reset0);
    put(t, fire_reset(v, h, v_th, v_reset, soft));
  }
  if (v_last) v_last[n] = v;
}

int launch_scalar(const float* x, void* spike, float* v_last, int T, int64_t N, int kind, float tau, float v_th, int soft_reset,
                  float v_reset, int spike_dtype, const float* W, const float* b, void* stream) {
  if (!x || !spike) return SDF_E_NULL;
  if (T < 1 || N < 1) return SDF_E_SHAPE;
  if (spike_dtype != SDF_F32 && spike_dtype != SDF_U8) return SDF_E_DTYPE;
  if (kind == SDF_PSN && (!W || !b)) return SDF_E_NULL;
  if (!sdf_tau_ok(kind, tau)) return SDF_E_SHAPE;
  const float inv_tau = sdf_inv_tau(kind, tau);
  SDF_LAUNCH(neuron_scalar_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, sdf_stream(stream), x, spike, v_last, T, N,
                     kind, tau, inv_tau, v_th, v_reset, soft_reset, spike_dtype, W, b);
  SDF_LAUNCH_CHECK();
  return 0;
}

// `glif`: the descriptor of sdf_glif_neuron_fwd - its T list, no v_last, and none of the neuron fields (kind, tau, psn_*) is read
// `vseq`: the descriptor of sdf_neuron_vseq_fwd - a PSN has no membrane and is refused where the kind is checked
int validate(const SdfNeuronDesc& d, bool glif = false, bool vseq = false) {
  if (!d.x || !d.out) return SDF_E_NULL;
  if (d.T < 1 || d.nb < 1 || d.ni < 4) return SDF_E_SHAPE;
  if (glif && (!sdf_in(SDF_T_GLIF, d.T) || d.v_last)) return SDF_E_SHAPE;
  if (d.out_dtype != SDF_F32 && d.out_dtype != SDF_U8) return SDF_E_DTYPE;
  if (!glif && d.kind != SDF_LIF && d.kind != SDF_PSN && d.kind != SDF_IF) return SDF_E_DTYPE;
  if (vseq && d.kind == SDF_PSN) return SDF_E_DTYPE;
  if (d.ni % 4 || d.o_sb % 4 || d.o_st % 4) return SDF_E_SHAPE;
  if (!sdf_aligned(d.x, 16) || !sdf_aligned(d.out, d.out_dtype == SDF_F32 ? 16 : 4)) return SDF_E_ALIGN;
  if (d.nrep < 0 || (d.nrep > 1 && (d.rowmap || d.x_srep % 4 || d.o_srep % 4))) return SDF_E_SHAPE;      // (the outer dimension is a dense-mode feature)
  if (d.rowmap) {
    if (d.rowlen < 4 || d.rowlen % 4 || (d.nb * d.ni) % d.rowlen) return SDF_E_SHAPE;
  } else if (d.x_sb % 4 || d.x_st % 4) {
    return SDF_E_SHAPE;
  }
  if (d.alpha) {
    if (!d.beta) return SDF_E_NULL;
    if (d.C < 1 || d.inner < 1) return SDF_E_SHAPE;
    if (d.inner == 1 ? (d.C % 4 != 0) : (d.inner % 4 != 0)) return SDF_E_SHAPE;
    if (d.inner == 1 && (!sdf_aligned(d.alpha, 16) || !sdf_aligned(d.beta, 16))) return SDF_E_ALIGN;
  }
  if (d.add && (d.add_period < 4 || d.add_period % 4 || d.add_st % 4 || !sdf_aligned(d.add, 16))) return SDF_E_SHAPE;
  if (glif) return 0;
  if (d.kind == SDF_PSN) {
    if (!d.psn_w || !d.psn_b) return SDF_E_NULL;
    if (d.v_last) return SDF_E_SHAPE;
  } else if (!sdf_tau_ok(d.kind, d.tau)) {
    return SDF_E_SHAPE;
  }
  if (d.v_last && !sdf_aligned(d.v_last, 16)) return SDF_E_ALIGN;
  return 0;
}

NeuronParams neuron_params(const SdfNeuronDesc& d) {               // of a validated descriptor
  NeuronParams P;
  P.d = d;
  P.quads = (d.nrep > 1 ? d.nrep : 1) * d.nb * d.ni / 4;
  P.rows = d.rowmap ? d.nb * d.ni / d.rowlen : 0;
  P.inv_tau = sdf_inv_tau(d.kind, d.tau);
  return P;
}

}  // namespace

extern "C" int sdf_neuron_fwd(const SdfNeuronDesc* dp, void* stream) {
  if (!dp) return SDF_E_NULL;
  int rc = validate(*dp);
  if (rc) return rc;
  const NeuronParams P = neuron_params(*dp);
  dim3 grid((unsigned)sdf_quad_blocks(P.quads * 4)), block(256);
  hipStream_t s = sdf_stream(stream);
  if (!sdf_dispatch(SDF_T_STREAM, dp->T, [&](auto tt) { SDF_LAUNCH(neuron_kernel<tt>, grid, block, 0, s, P); })) {
    if (dp->kind == SDF_PSN) return SDF_E_SHAPE;
    SDF_LAUNCH(neuron_kernel<0>, grid, block, 0, s, P);            // any other T: the runtime-T kernel
  }
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_glif_neuron_fwd(const SdfNeuronDesc* dp, const float* tab, void* stream) {
  if (!dp || !tab) return SDF_E_NULL;
  int rc = validate(*dp, true);
  if (rc) return rc;
  if (!sdf_aligned(tab, 4)) return SDF_E_ALIGN;
  NeuronParams P = neuron_params(*dp);
  if (sdf_quad_blocks(P.quads * 4) >= (1LL << 31)) return SDF_E_SHAPE;
  dim3 grid((unsigned)sdf_quad_blocks(P.quads * 4)), block(256);
  hipStream_t s = sdf_stream(stream);
  sdf_dispatch(SDF_T_GLIF, dp->T, [&](auto tt) { SDF_LAUNCH(glif_neuron_kernel<tt>, grid, block, 0, s, P, tab); });   // (validated: T is in the list)
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_neuron_vseq_fwd(const SdfNeuronDesc* dp, float* v_seq, void* stream) {
  if (!dp || !v_seq) return SDF_E_NULL;
  int rc = validate(*dp, false, true);
  if (rc) return rc;
  if (!sdf_aligned(v_seq, 16)) return SDF_E_ALIGN;
  const NeuronParams P = neuron_params(*dp);
  if (sdf_quad_blocks(P.quads * 4) >= (1LL << 31)) return SDF_E_SHAPE;
  dim3 grid((unsigned)sdf_quad_blocks(P.quads * 4)), block(256);
  hipStream_t s = sdf_stream(stream);
  if (!sdf_dispatch(SDF_T_GLIF, dp->T, [&](auto tt) { SDF_LAUNCH(neuron_vseq_kernel<tt>, grid, block, 0, s, P, v_seq); }))
    SDF_LAUNCH(neuron_vseq_kernel<0>, grid, block, 0, s, P, v_seq);   // any other T: the runtime-T form
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_neuron_multi_fwd(const SdfNeuronDesc* descs, int n, void* stream) {
  if (!descs) return SDF_E_NULL;
  if (n < 1) return SDF_E_SHAPE;
  if (n == 1) return sdf_neuron_fwd(descs, stream);
  const int T = descs[0].T;
  bool one = n <= MULTI_MAX && sdf_in(SDF_T_GLIF, T);
  for (int i = 0; i < n; ++i) {
    const int rc = validate(descs[i]);
    if (rc) return rc;
    one = one && descs[i].T == T;
  }
  if (!one) {                                                    // mixed T or more than MULTI_MAX descriptors: one launch each
    for (int i = 0; i < n; ++i) {
      const int rc = sdf_neuron_fwd(descs + i, stream);
      if (rc) return rc;
    }
    return 0;
  }
  NeuronMulti M;
  M.n = n;
  int64_t wgs = 0;
  for (int i = 0; i < n; ++i) {
    M.p[i] = neuron_params(descs[i]);
    M.first[i] = (int)wgs;
    wgs += sdf_quad_blocks(M.p[i].quads * 4);
    if (wgs >= (1LL << 31)) return SDF_E_SHAPE;
  }
  for (int i = n; i <= MULTI_MAX; ++i) M.first[i] = (int)wgs;
  dim3 grid((unsigned)wgs), block(256);
  hipStream_t s = sdf_stream(stream);
  sdf_dispatch(SDF_T_GLIF, T, [&](auto tt) { SDF_LAUNCH(neuron_multi_kernel<tt>, grid, block, 0, s, M); });   // `one`: T is in the list
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_lif_fwd(const float* x, void* spike, float* v_last, int T, int64_t N, float tau, float v_th,
                           int soft_reset, float v_reset, int spike_dtype, void* stream) {
  if (N % 4) return launch_scalar(x, spike, v_last, T, N, SDF_LIF, tau, v_th, soft_reset, v_reset, spike_dtype, nullptr, nullptr, stream);
  SdfNeuronDesc d = {};
  d.x = x; d.out = spike; d.v_last = v_last; d.T = T; d.out_dtype = spike_dtype;
  d.nb = 1; d.ni = N; d.x_sb = 0; d.x_st = N; d.o_sb = 0; d.o_st = N;
  d.kind = SDF_LIF; d.tau = tau; d.v_th = v_th; d.v_reset = v_reset; d.soft_reset = soft_reset;
  return sdf_neuron_fwd(&d, stream);
}

extern "C" int sdf_psn_fwd(const float* x, const float* W, const float* b, void* spike, int T, int64_t N,
                           int spike_dtype, void* stream) {
  if (N % 4 || !sdf_in(SDF_T_STREAM, T))
    return launch_scalar(x, spike, nullptr, T, N, SDF_PSN, 2.f, 0.f, 1, 0.f, spike_dtype, W, b, stream);
  SdfNeuronDesc d = {};
  d.x = x; d.out = spike; d.T = T; d.out_dtype = spike_dtype;
  d.nb = 1; d.ni = N; d.x_sb = 0; d.x_st = N; d.o_sb = 0; d.o_st = N;
  d.kind = SDF_PSN; d.psn_w = W; d.psn_b = b;
  return sdf_neuron_fwd(&d, stream);
}

namespace {

// Training-path PLIF forward: the multiplier k = sigmoid(w) is read from device memory (one fp32 scalar, written by the caller's
// sigmoid on the same stream), so a train step needs no host read-back per neuron.  Arithmetic = lif_charge with inv_tau = k
// (plif_charge's single multiply costs this kernel a register, and a wave per SIMD at T = 16).
template <int TT>
__global__ __launch_bounds__(256) void plif_fwd_kernel(const float* x, const float* kp, float* spike, int64_t N, float v_th,
                                                       int soft_reset, float v_reset) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= N) return;
  const int64_t e = q * 4;
  float4 xv[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) xv[t] = load4(x + (int64_t)t * N + e);
  const float k = *kp;
  const bool soft = soft_reset != 0, reset0 = soft || v_reset == 0.f;
  const float v0 = soft ? 0.f : v_reset;
  float4 v = make_float4(v0, v0, v0, v0);
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    float4 h, s;
    h.x = lif_charge(v.x, xv[t].x, __builtin_inff(), k, v_reset, reset0);
    h.y = lif_charge(v.y, xv[t].y, __builtin_inff(), k, v_reset, reset0);
    h.z = lif_charge(v.z, xv[t].z, __builtin_inff(), k, v_reset, reset0);
    h.w = lif_charge(v.w, xv[t].w, __builtin_inff(), k, v_reset, reset0);
    s.x = fire_reset(v.x, h.x, v_th, v_reset, soft);
    s.y = fire_reset(v.y, h.y, v_th, v_reset, soft);
    s.z = fire_reset(v.z, h.z, v_th, v_reset, soft);
    s.w = fire_reset(v.w, h.w, v_th, v_reset, soft);
    *reinterpret_cast<float4*>(spike + (int64_t)t * N + e) = s;
  }
}

}  // namespace

extern "C" int sdf_plif_fwd(const float* x, const float* plif_k, float* spike, int T, int64_t N, float v_th, int soft_reset,
                            float v_reset, void* stream) {
  if (!x || !plif_k || !spike) return SDF_E_NULL;
  if (N < 4 || N % 4) return SDF_E_SHAPE;
  if (!sdf_aligned(x, 16) || !sdf_aligned(spike, 16) || !sdf_aligned(plif_k, 4)) return SDF_E_ALIGN;
  if (soft_reset) v_reset = 0.f;
  dim3 grid((unsigned)sdf_quad_blocks(N)), block(256);
  hipStream_t s = sdf_stream(stream);
  if (!sdf_dispatch(SDF_T_STREAM, T, [&](auto tt) {
        SDF_LAUNCH(plif_fwd_kernel<tt>, grid, block, 0, s, x, plif_k, spike, N, v_th, soft_reset, v_reset);
      }))
    return SDF_E_SHAPE;
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdf_version(void) { return SDF_VERSION; }
