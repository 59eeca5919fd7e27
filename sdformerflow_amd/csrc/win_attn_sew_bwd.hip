// Backward of the SEW spiking window attention (the core sdf_win_attn_fwd computes in SDF_ATTN_SEW mode), gfx950.
//
// Per window b and head g (reference models/STSwinNet_SNN/Spiking_swin_transformer3D.py:320-363; no softmax):
//   A = scale[g] Q K^T + bias[g] (+ mask[b % nW]),  O = A V
// with Q, K, V the raw head view (B_, nH, N, 32) of the (T', B_, N1, C) spike buffers and O leaving through the
// (B_, nH, T', N1, hd) -> (T', B_, N1, C) scramble.  Given dO in that scrambled layout, dA = dO V^T exactly, and by associativity:
//   dQ = scale dO (V^T K),   dK = scale V (dO^T Q),   dV = scale K (Q^T dO) + (bias[g] + mask)^T dO,
//   d_bias[g] = sum over windows of dO V^T  (the mask gets no gradient).
// Only the (bias + mask)^T dO term and d_bias need N x N work; the rest goes through two 32 x 32 Gram matrices.
//
// sew_bwd_kernel: one workgroup (4 waves) per (window, head).  Q, K, V staged in LDS as bytes, dO as fp32; the Grams V^T K and Q^T dO
//   (Q^T dO is also (dO^T Q)^T) land in LDS; dQ and dK follow from them; dV walks 32-key tiles of (bias + mask), staged in LDS.
// sew_bwd_dbias_kernel: d_bias as split-K partials - a workgroup owns 16 query rows of one head and a fixed run of windows, and
//   accumulates dO V^T for them in registers; sew_bwd_dbias_finish_kernel adds the runs in run order.  No (B_, nH, N, N) slab, no
//   float atomics: two calls give bit-equal results.
// Arithmetic: fp32 FMA on the vector ALU throughout (the spikes are exact 0 / 1, dO and the Grams stay fp32; on gfx950 the fp32 vector
// rate equals the exact fp32 MFMA rate, MI355X_MICROARCH: 157.3 TFLOPS).
// The head dimension, the spike unpack u8x4_f and dout_row (the forward's output scramble) are win_attn_common.h's.
#include "win_attn_common.h"

namespace {

constexpr int NMAX = 192;             // the forward's limit (12 tiles of 16 tokens)
constexpr int LDO = HD + 1;           // padded fp32 row of dO (floats)
constexpr int LDG = HD + 4;           // Gram row (floats; float4 reads)
constexpr int MT = 32;                // keys per (bias + mask) tile
constexpr int LDB = MT + 1;
constexpr int RT = 16;                // query rows per d_bias workgroup
constexpr int LDV = HD + 4;           // fp32 row of V in the d_bias kernel (float4 reads)
constexpr int DBIAS_TARGET_WG = 2048; // grid the d_bias split aims for

// windows per d_bias run: a function of the shape only, so the summation order is too
__host__ __device__ inline int dbias_run(int B_, int nH, int N) {
  const int tiles = nH * ((N + RT - 1) / RT);
  int runs = (DBIAS_TARGET_WG + tiles - 1) / tiles;
  if (runs > B_) runs = B_;
  if (runs < 1) runs = 1;
  return (B_ + runs - 1) / runs;
}
__host__ __device__ inline int dbias_runs(int B_, int nH, int N) {
  const int w = dbias_run(B_, nH, N);
  return (B_ + w - 1) / w;
}

__host__ __device__ inline int dO_floats(int N) { return (N * LDO + 3) & ~3; }     // keeps the Grams behind it 16-byte aligned

size_t main_lds_bytes(int N) {
  return (size_t)3 * N * HD + (size_t)(dO_floats(N) + 2 * HD * LDG + N * LDB) * sizeof(float);
}

__global__ __launch_bounds__(256) void sew_bwd_kernel(SdfWinAttnSewBwdDesc d) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int N = d.N1 * d.Tq, nH = d.nH;
  const int bg = blockIdx.x, b = bg / nH, g = bg - b * nH;
  const int tid = threadIdx.x;
  // fp32 regions first (16-byte aligned), then the byte planes
  float* dO = reinterpret_cast<float*>(lds);                    // (N, LDO)
  float* G1 = dO + dO_floats(N);                               // V^T K  (HD, LDG)
  float* G3 = G1 + HD * LDG;                                    // Q^T dO (HD, LDG)
  float* BM = G3 + HD * LDG;                                    // (N, LDB): bias + mask, one key tile
  unsigned char* Qs = reinterpret_cast<unsigned char*>(BM + N * LDB);
  unsigned char* Ks = Qs + N * HD;
  unsigned char* Vs = Ks + N * HD;

  const int64_t head_off = (int64_t)bg * N * HD;                // raw head view: (b, g) is one contiguous N x 32 block
  {
    const uint32_t* q4 = reinterpret_cast<const uint32_t*>(d.q + head_off);
    const uint32_t* k4 = reinterpret_cast<const uint32_t*>(d.k + head_off);
    const uint32_t* v4 = reinterpret_cast<const uint32_t*>(d.v + head_off);
    uint32_t* Q4 = reinterpret_cast<uint32_t*>(Qs);
    uint32_t* K4 = reinterpret_cast<uint32_t*>(Ks);
    uint32_t* V4 = reinterpret_cast<uint32_t*>(Vs);
    for (int i = tid; i < N * HD / 4; i += 256) {
      Q4[i] = q4[i];
      K4[i] = k4[i];
      V4[i] = v4[i];
    }
    for (int i = tid; i < N * (HD / 4); i += 256) {
      const int n = i >> 3, e4 = (i & 7) * 4;
      const float4 x = *reinterpret_cast<const float4*>(dout_row(d, b, g, n) + e4);
      float* r = dO + n * LDO + e4;
      r[0] = x.x;
      r[1] = x.y;
      r[2] = x.z;
      r[3] = x.w;
    }
  }
  __syncthreads();

  const int r8 = tid >> 3, e0 = (tid & 7) * 4;                  // 32 rows x 8 column quads
  // ---- Grams: G1[r][e] = sum_n V[n][r] K[n][e],  G3[r][e] = sum_n Q[n][r] dO[n][e] ----
  {
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a3[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) {
      const float vr = (float)Vs[n * HD + r8], qr = (float)Qs[n * HD + r8];
      const float4 kk = u8x4_f(*reinterpret_cast<const uint32_t*>(Ks + n * HD + e0));
      const float* o = dO + n * LDO + e0;
      a1[0] = fmaf(vr, kk.x, a1[0]);
      a1[1] = fmaf(vr, kk.y, a1[1]);
      a1[2] = fmaf(vr, kk.z, a1[2]);
      a1[3] = fmaf(vr, kk.w, a1[3]);
      a3[0] = fmaf(qr, o[0], a3[0]);
      a3[1] = fmaf(qr, o[1], a3[1]);
      a3[2] = fmaf(qr, o[2], a3[2]);
      a3[3] = fmaf(qr, o[3], a3[3]);
    }
    *reinterpret_cast<float4*>(G1 + r8 * LDG + e0) = make_float4(a1[0], a1[1], a1[2], a1[3]);
    *reinterpret_cast<float4*>(G3 + r8 * LDG + e0) = make_float4(a3[0], a3[1], a3[2], a3[3]);
  }
  __syncthreads();

  const float sc = d.scale[g];
  // ---- dQ[n][e] = scale sum_r dO[n][r] G1[r][e];  dK[n][e] = scale sum_r V[n][r] G3[e][r] ----
  for (int n = r8; n < N; n += 32) {
    float aq[4] = {0.f, 0.f, 0.f, 0.f}, ak[4] = {0.f, 0.f, 0.f, 0.f};
    const float* o = dO + n * LDO;
    const unsigned char* vrow = Vs + n * HD;
#pragma unroll 8
    for (int r = 0; r < HD; ++r) {
      const float4 g1 = *reinterpret_cast<const float4*>(G1 + r * LDG + e0);
      const float on = o[r], vn = (float)vrow[r];
      aq[0] = fmaf(on, g1.x, aq[0]);
      aq[1] = fmaf(on, g1.y, aq[1]);
      aq[2] = fmaf(on, g1.z, aq[2]);
      aq[3] = fmaf(on, g1.w, aq[3]);
      ak[0] = fmaf(vn, G3[(e0 + 0) * LDG + r], ak[0]);
      ak[1] = fmaf(vn, G3[(e0 + 1) * LDG + r], ak[1]);
      ak[2] = fmaf(vn, G3[(e0 + 2) * LDG + r], ak[2]);
      ak[3] = fmaf(vn, G3[(e0 + 3) * LDG + r], ak[3]);
    }
    const int64_t off = head_off + (int64_t)n * HD + e0;
    *reinterpret_cast<float4*>(d.dq + off) = make_float4(sc * aq[0], sc * aq[1], sc * aq[2], sc * aq[3]);
    *reinterpret_cast<float4*>(d.dk + off) = make_float4(sc * ak[0], sc * ak[1], sc * ak[2], sc * ak[3]);
  }

  // ---- dV[m][e] = scale sum_r K[m][r] G3[r][e] + sum_n (bias + mask)[n][m] dO[n][e], 32 keys per tile ----
  const float* bias = d.bias + (int64_t)g * N * N;
  const float* mask = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
  for (int m0 = 0; m0 < N; m0 += MT) {
    __syncthreads();                                            // the previous tile is read out
    for (int i = tid; i < N * MT; i += 256) {
      const int n = i / MT, j = i - n * MT, m = m0 + j;
      float x = 0.f;
      if (m < N) {
        x = bias[(int64_t)n * N + m];
        if (mask) x += mask[(int64_t)n * N + m];
      }
      BM[n * LDB + j] = x;
    }
    __syncthreads();
    const int m = m0 + r8;
    if (m < N) {
      float ag[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
      const unsigned char* krow = Ks + m * HD;
#pragma unroll 8
      for (int r = 0; r < HD; ++r) {
        const float4 g3 = *reinterpret_cast<const float4*>(G3 + r * LDG + e0);
        const float kn = (float)krow[r];
        ag[0] = fmaf(kn, g3.x, ag[0]);
        ag[1] = fmaf(kn, g3.y, ag[1]);
        ag[2] = fmaf(kn, g3.z, ag[2]);
        ag[3] = fmaf(kn, g3.w, ag[3]);
      }
      for (int n = 0; n < N; ++n) {
        const float w = BM[n * LDB + r8];
        const float* o = dO + n * LDO + e0;
        ab[0] = fmaf(w, o[0], ab[0]);
        ab[1] = fmaf(w, o[1], ab[1]);
        ab[2] = fmaf(w, o[2], ab[2]);
        ab[3] = fmaf(w, o[3], ab[3]);
      }
      const int64_t off = head_off + (int64_t)m * HD + e0;
      *reinterpret_cast<float4*>(d.dv + off) =
          make_float4(fmaf(sc, ag[0], ab[0]), fmaf(sc, ag[1], ab[1]), fmaf(sc, ag[2], ab[2]), fmaf(sc, ag[3], ab[3]));
    }
  }
}

// d_bias partial of one run of windows: rows n0 .. n0+RT-1 of head g, every key m.  blockDim = N rounded up to 64; thread = key m.
__global__ __launch_bounds__(256) void sew_bwd_dbias_kernel(SdfWinAttnSewBwdDesc d, float* part, int wrun) {
  __shared__ __align__(16) float Vf[NMAX * LDV];
  __shared__ __align__(16) float Or[RT * HD];
  const int N = d.N1 * d.Tq, nH = d.nH;
  const int run = blockIdx.x, g = blockIdx.y, n0 = blockIdx.z * RT;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int rows = min(RT, N - n0);
  const int b0 = run * wrun, b1 = min(d.B_, b0 + wrun);
  float acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = 0.f;
  for (int b = b0; b < b1; ++b) {
    __syncthreads();                                            // the previous window is read out
    const uint32_t* v4 = reinterpret_cast<const uint32_t*>(d.v + ((int64_t)b * nH + g) * N * HD);
    for (int i = tid; i < N * HD / 4; i += nthr) {
      const int n = i >> 3, e4 = (i & 7) * 4;
      *reinterpret_cast<float4*>(Vf + n * LDV + e4) = u8x4_f(v4[i]);
    }
    for (int i = tid; i < RT * (HD / 4); i += nthr) {
      const int r = i >> 3, e4 = (i & 7) * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) x = *reinterpret_cast<const float4*>(dout_row(d, b, g, n0 + r) + e4);
      *reinterpret_cast<float4*>(Or + r * HD + e4) = x;
    }
    __syncthreads();
    if (tid < N) {
      const float* vrow = Vf + tid * LDV;
#pragma unroll 2
      for (int e = 0; e < HD; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(vrow + e);
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          const float4 o = *reinterpret_cast<const float4*>(Or + r * HD + e);
          acc[r] = fmaf(o.x, v.x, acc[r]);
          acc[r] = fmaf(o.y, v.y, acc[r]);
          acc[r] = fmaf(o.z, v.z, acc[r]);
          acc[r] = fmaf(o.w, v.w, acc[r]);
        }
      }
    }
  }
  if (tid < N) {
    float* p = part + (((int64_t)run * nH + g) * N + n0) * N + tid;
    for (int r = 0; r < rows; ++r) p[(int64_t)r * N] = acc[r];
  }
}

// d_bias (nH, N, N) = the runs' partials added in run order.  One thread per element.
__global__ __launch_bounds__(256) void sew_bwd_dbias_finish_kernel(const float* part, float* d_bias, int64_t nb, int runs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nb) return;
  float s = 0.f;
  for (int r = 0; r < runs; ++r) s += part[(int64_t)r * nb + idx];
  d_bias[idx] = s;
}

bool shape_ok(int B_, int nH, int Tq, int N1, int hd) {
  return hd == HD && B_ >= 1 && nH >= 1 && Tq >= 1 && N1 >= 1 && Tq * N1 <= NMAX;
}

}  // namespace

extern "C" int64_t sdf_win_attn_sew_bwd_workspace_bytes(int B_, int nH, int N) {
  if (B_ < 1 || nH < 1 || N < 1 || N > NMAX) return 0;
  return align256((int64_t)dbias_runs(B_, nH, N) * nH * N * N * 4);
}

extern "C" int sdf_win_attn_sew_bwd(const SdfWinAttnSewBwdDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (!d->q || !d->k || !d->v || !d->dout || !d->scale || !d->bias || !d->dq || !d->dk || !d->dv || !d->d_bias || !d->workspace)
    return SDF_E_NULL;
  if (!shape_ok(d->B_, d->nH, d->Tq, d->N1, d->hd)) return SDF_E_SHAPE;
  if (d->mask && (d->nW < 1 || d->B_ % d->nW)) return SDF_E_SHAPE;
  const int N = d->Tq * d->N1;
  if (d->workspace_bytes < sdf_win_attn_sew_bwd_workspace_bytes(d->B_, d->nH, N)) return SDF_E_SHAPE;
  if (!sdf_aligned(d->q, 4) || !sdf_aligned(d->k, 4) || !sdf_aligned(d->v, 4) || !sdf_aligned(d->dout, 16) ||
      !sdf_aligned(d->dq, 16) || !sdf_aligned(d->dk, 16) || !sdf_aligned(d->dv, 16) || !sdf_aligned(d->workspace, 256))
    return SDF_E_ALIGN;
  SdfWinAttnSewBwdDesc P = *d;
  if (!d->mask) P.nW = 1;
  static std::atomic<uint64_t> opt{0};                          // > 64 KiB of dynamic LDS at the largest windows: opt-in once per device
  if (const int e = sdf_lds_opt_in(opt, reinterpret_cast<const void*>(sew_bwd_kernel), (int)main_lds_bytes(NMAX))) return e;
  hipStream_t s = sdf_stream(stream);
  SDF_LAUNCH(sew_bwd_kernel, dim3((unsigned)((int64_t)d->B_ * d->nH)), dim3(256), main_lds_bytes(N), s, P);
  SDF_LAUNCH_CHECK();
  const int wrun = dbias_run(d->B_, d->nH, N), runs = dbias_runs(d->B_, d->nH, N);
  float* part = reinterpret_cast<float*>(d->workspace);
  const dim3 grid((unsigned)runs, (unsigned)d->nH, (unsigned)((N + RT - 1) / RT));
  SDF_LAUNCH(sew_bwd_dbias_kernel, grid, dim3((unsigned)((N + 63) / 64 * 64)), 0, s, P, part, wrun);
  SDF_LAUNCH_CHECK();
  const int64_t nb = (int64_t)d->nH * N * N;
  SDF_LAUNCH(sew_bwd_dbias_finish_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, part, d->d_bias, nb, runs);
  SDF_LAUNCH_CHECK();
  return 0;
}
