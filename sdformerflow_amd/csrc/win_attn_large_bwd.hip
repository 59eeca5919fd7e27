// Backward of the window attention for windows of 193 .. 1024 tokens (up to (2,22,22)), gfx950: the arithmetic of win_attn_bwd.hip (ANN:
// cosine scores, softmax) and win_attn_sew_bwd.hip (SEW: byte spikes, no softmax), with keys and queries walked in blocks of 64 tokens
// staged in LDS instead of a whole window held there.  Nothing of the LDS or register budget depends on N (at most 38 912 B of static LDS per workgroup),
// no buffer of the workspace grows as B_ nH N^2, no float atomics: every cross-window sum has a fixed order, two calls are bit-equal.
//
// ANN, per window b and head g (formulas: win_attn_bwd.hip).  Every product is the exact fp32 MFMA; the score is rounded as
// (acc * scale + bias) + mask; a key past N scores -inf (P = 0); bias and mask are finite.
//   win_attn_large_ann_bwd_query_kernel  workgroup = (window, head, 64 queries), one 16-query tile per wave, two key walks:
//     walk 1: S^T = K^ Q^^T and dP^T = V dO^T per 64-key block, online softmax -> row maximum m, 1 / row sum and
//             D = rowsum(P o dP) (= dO . O: carried through the walk as sum e dP, rescaled with the row sum), kept in registers and
//             stored per query in the workspace for the other kernels;
//     walk 2: P = exp(S - m) / l, dS = P o (dP - D), U += dS K^; then dq^ = scale U, the d_scale term sum q^ . U and the
//             F.normalize backward once the row is complete.
//   win_attn_large_ann_bwd_key_kernel    workgroup = (window, head, 64 keys), one 16-key tile per wave, a walk over 64-query blocks
//     (q^, dO and the stored row statistics staged): dv += P^T dO, dk^ += scale dS^T Q^, then the normalize backward.
//   win_attn_large_ann_bwd_dbias_kernel  d_bias as split-K partials: a workgroup owns (head, 64 queries, 64 keys) and a fixed run of
//     windows, recomputes dS of that tile for each of them from the stored row statistics and adds it up in registers;
//     win_attn_large_bwd_sum_runs_kernel adds the runs in run order.
//   win_attn_large_ann_bwd_reduce_kernel d_scale and d_pad: the per-workgroup partials in (window, group) order.
// QK^T is therefore recomputed four times (two query walks, the key walk, d_bias) and V dO^T four times.
//
// SEW, per window b and head g (formulas: win_attn_sew_bwd.hip; fp32 FMA on the vector ALU, spikes exact):
//   win_attn_large_sew_bwd_gram_kernel   workgroup = (window, head): the Grams V^T K and Q^T dO over 64-token blocks, then dQ and dK
//     over 64-token blocks; Q^T dO (32 x 32) is kept in the workspace.
//   win_attn_large_sew_bwd_dv_kernel     workgroup = (window, head, 64 keys): dV from Q^T dO and the (bias + mask)^T dO walk, with
//     (bias + mask) and dO streamed in 64-query blocks.
//   win_attn_large_sew_dbias_kernel      split-K over runs of windows as sew_bwd_dbias_kernel, V staged per 256-key block.
// token_row, norm_bwd, sum16, norm_row8, load_row8 / mfma_row8, the score rounding, u8x4_f, dout_row and the workspace helpers are
// win_attn_common.h's.
#include "win_attn_common.h"

namespace {

constexpr int N_ABOVE = 192, N_MAX = 1024;   // served: N_ABOVE < N <= N_MAX (up to N_ABOVE: sdf_win_attn_ann_bwd / sdf_win_attn_sew_bwd)
constexpr int TB = 64;                       // tokens per staged block = tokens a workgroup owns
constexpr int RQ = HD + 1;                   // query kernel's partials per workgroup: d_pad (q of one head) + d_scale
constexpr int RK = 2 * HD;                   // key kernel's: d_pad (k | v of one head)
constexpr int DBIAS_TARGET_WG = 2048;        // grid the d_bias splits aim for

__host__ __device__ inline int groups_of(int N) { return (N + TB - 1) / TB; }

// windows per d_bias run and the number of runs: functions of the shape only, so the summation order is too
__host__ __device__ inline int dbias_run(int B_, int tiles) {
  int runs = (DBIAS_TARGET_WG + tiles - 1) / tiles;
  if (runs > B_) runs = B_;
  if (runs < 1) runs = 1;
  return (B_ + runs - 1) / runs;
}
__host__ __device__ inline int dbias_runs(int B_, int tiles) {
  const int w = dbias_run(B_, tiles);
  return (B_ + w - 1) / w;
}

// d_bias (nH, N, N) = the runs' partials added in run order.  One thread per element.
__global__ __launch_bounds__(256) void win_attn_large_bwd_sum_runs_kernel(const float* part, float* d_bias, int64_t nb, int runs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nb) return;
  float s = 0.f;
  for (int r = 0; r < runs; ++r) s += part[(int64_t)r * nb + idx];
  d_bias[idx] = s;
}

// =====================================================================================================================================
// ANN
// =====================================================================================================================================
struct AnnBwdParams {
  SdfWinAttnBwdDesc d;
  float* ws_m;          // (B_, nH, NP) each: row maximum, 1 / row sum, D of every query
  float* ws_l;
  float* ws_D;
  float* ws_q;          // (B_, nH, G, RQ): d_pad of q (32) and the d_scale term of a query group
  float* ws_kv;         // (B_, nH, G, RK): d_pad of k | v of a key group
  float* ws_part;       // (runs, nH, N, N): d_bias partials
  int wrun;             // windows per run
};

// Stage tokens t0 .. t0 + 63 of (window b, head g) as dst[64][LDW]: PART 0 / 1 / 2 = q / k / v of the token's qkv row (a padding
// token reads pad_qkv), PART 3 = dO (zero for a padding token: its output is cropped).  NORM: the row L2-normalised as the forward
// does, its raw norm to nrm[64] where the caller keeps it (nrm may be null).  Tokens past N are zero rows.  All 256 threads: 8 lanes per row (one float4 each), 32 rows per pass.
template <int PART, bool NORM>
__device__ __forceinline__ void stage_rows(const SdfWinAttnBwdDesc& d, int b, int g, int t0, float* dst, float* nrm, int tid) {
  const int C = d.nH * HD, piece = tid & 7;
#pragma unroll
  for (int it = 0; it < TB / 32; ++it) {
    const int r = (tid >> 3) + 32 * it, t = t0 + r;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < d.N) {
      const int64_t row = token_row(d, b, t);
      if (PART < 3) {
        const float* base = (row >= 0 ? d.qkv + row * 3 * (int64_t)C : d.pad_qkv) + PART * C + g * HD + 4 * piece;
        x = *reinterpret_cast<const float4*>(base);
      } else if (row >= 0) {
        x = *reinterpret_cast<const float4*>(d.dout + row * C + g * HD + 4 * piece);
      }
    }
    if (NORM) {                                          // (win_attn_common.h norm_row8)
      const float n = norm_row8(x);
      if (nrm && piece == 0) nrm[r] = n;
    }
    *reinterpret_cast<float4*>(&dst[r * LDW + 4 * piece]) = x;
  }
}

// Score and dP strip of one 16-query tile against the staged 64-key block: st[jt][r] = S[qi][kb0 + 16 jt + 4 lg + r] (scaled, bias and
// mask added; -inf for a key past N), dp[jt][r] = dP of the same element.  qreg / greg = q^ / dO of query qi, dims 8 lg .. 8 lg + 7.
__device__ __forceinline__ void score_strip(const float* Ks, const float* Vs, const float (&qreg)[8], const float (&greg)[8], int qi,
                                            int kb0, int N, float ls, const float* bias_g, const float* mask_w, int l15, int lg,
                                            f32x4 (&st)[TB / 16], f32x4 (&dp)[TB / 16]) {
#pragma unroll
  for (int jt = 0; jt < TB / 16; ++jt) {
    const int kj = jt * 16 + l15;                        // A operand row: key (inside the block)
    f32x4 acc = mfma_row8(&Ks[kj * LDW + 8 * lg], qreg);
    dp[jt] = mfma_row8(&Vs[kj * LDW + 8 * lg], greg);
    const int kb = kb0 + jt * 16 + 4 * lg;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = qi < N && kb + r < N;
      const float bv = ok ? bias_g[(int64_t)qi * N + kb + r] : 0.f;
      const float mv = (ok && mask_w) ? mask_w[(int64_t)qi * N + kb + r] : 0.f;
      acc[r] = attn_score(acc[r], ls, bv, mv, kb + r < N, -INFINITY);
    }
    st[jt] = acc;
  }
}

__global__ __launch_bounds__(256) void win_attn_large_ann_bwd_query_kernel(AnnBwdParams P) {
  __shared__ __attribute__((aligned(16))) float Qs[TB * LDW];      // q^ of this workgroup's queries
  __shared__ __attribute__((aligned(16))) float Gs[TB * LDW];      // dO of them
  __shared__ __attribute__((aligned(16))) float Ks[TB * LDW];      // k^ of the current key block
  __shared__ __attribute__((aligned(16))) float Vs[TB * LDW];      // v of it
  __shared__ float qn[TB];                                         // |q| of the queries
  __shared__ float red[4 * RQ];
  const SdfWinAttnBwdDesc& d = P.d;
  const int N = d.N, NP = padded_n(N), G = groups_of(N);
  const int bg = blockIdx.x / G, qg = blockIdx.x - bg * G;
  const int b = bg / d.nH, g = bg - b * d.nH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int C = d.nH * HD;
  const int64_t C3 = 3 * (int64_t)C;
  const int q0 = qg * TB;
  const int qt0 = q0 + wave * 16;                        // first query of this wave's tile
  const bool active = qt0 < N;                           // (a wave without a tile still stages and meets the barriers)
  const int qi = qt0 + l15;                              // this lane's query (column of the S^T tiles)

  stage_rows<0, true>(d, b, g, q0, Qs, qn, tid);
  stage_rows<3, false>(d, b, g, q0, Gs, nullptr, tid);
  __syncthreads();
  float qreg[8], greg[8];
  load_row8(&Qs[(wave * 16 + l15) * LDW + 8 * lg], qreg);
  load_row8(&Gs[(wave * 16 + l15) * LDW + 8 * lg], greg);

  const float ls = d.scale[g];
  const float* bias_g = d.bias + (int64_t)g * N * N;
  const float* mask_w = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
  const int nblk = groups_of(N);

  // ---- walk 1: row statistics through the online softmax ----
  float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;     // running maximum, sum of e, sum of e dP
  for (int blk = 0; blk < nblk; ++blk) {
    __syncthreads();                                     // every wave is done with the previous block
    stage_rows<1, true>(d, b, g, blk * TB, Ks, nullptr, tid);
    stage_rows<2, false>(d, b, g, blk * TB, Vs, nullptr, tid);
    __syncthreads();
    if (!active) continue;
    f32x4 st[TB / 16], dp[TB / 16];
    score_strip(Ks, Vs, qreg, greg, qi, blk * TB, N, ls, bias_g, mask_w, l15, lg, st, dp);
    float bm = st[0][0];                                 // the block's first key is a real key: finite
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) bm = fmaxf(fmaxf(fmaxf(bm, st[jt][0]), fmaxf(st[jt][1], st[jt][2])), st[jt][3]);
    bm = fmaxf(bm, __shfl_xor(bm, 16));
    bm = fmaxf(bm, __shfl_xor(bm, 32));
    const float m_new = fmaxf(m_run, bm);
    const float alpha = (m_run == -INFINITY) ? 0.f : expf(m_run - m_new);     // first block: nothing to scale
    float psum = 0.f, dsum = 0.f;
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = expf(st[jt][r] - m_new);         // a key past N: exp(-inf) = 0
        psum += e;
        dsum += e * dp[jt][r];
      }
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    dsum += __shfl_xor(dsum, 16);
    dsum += __shfl_xor(dsum, 32);
    l_run = l_run * alpha + psum;
    d_run = d_run * alpha + dsum;
    m_run = m_new;
  }
  const float inv = active ? 1.f / l_run : 0.f;
  const float Dq = d_run * inv;
  if (active && lg == 0) {                               // qi < NP: the statistics buffers hold NP rows
    const int64_t so = (int64_t)bg * NP + qi;
    P.ws_m[so] = m_run;
    P.ws_l[so] = inv;
    P.ws_D[so] = Dq;
  }

  // ---- walk 2: U = dS K^ ----
  f32x4 u0 = {0.f, 0.f, 0.f, 0.f}, u1 = {0.f, 0.f, 0.f, 0.f};
  for (int blk = 0; blk < nblk; ++blk) {
    __syncthreads();
    stage_rows<1, true>(d, b, g, blk * TB, Ks, nullptr, tid);
    stage_rows<2, false>(d, b, g, blk * TB, Vs, nullptr, tid);
    __syncthreads();
    if (!active) continue;
    f32x4 st[TB / 16], dp[TB / 16];
    score_strip(Ks, Vs, qreg, greg, qi, blk * TB, N, ls, bias_g, mask_w, l15, lg, st, dp);
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(st[jt][r] - m_run) * inv;
        st[jt][r] = p * (dp[jt][r] - Dq);                // dS in place of S
      }
    }
    // A = dS (registers), B = K^[key = 16 jt + 4 lg + s][dim = 16 dt + l15]
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int key = jt * 16 + 4 * lg + s;
        u0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][s], Ks[key * LDW + l15], u0, 0, 0, 0);
        u1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][s], Ks[key * LDW + 16 + l15], u1, 0, 0, 0);
      }
    }
  }

  // u[r] = U[query qt0 + 4 lg + r][dim l15 | 16 + l15]: d_scale term, dq^ = scale U, normalize backward, store
  float pq0 = 0.f, pq1 = 0.f, sacc = 0.f;
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int il = wave * 16 + 4 * lg + r, i = q0 + il;
      const float y0 = Qs[il * LDW + l15], y1 = Qs[il * LDW + 16 + l15];
      sacc += y0 * u0[r] + y1 * u1[r];
      const float dy0 = ls * u0[r], dy1 = ls * u1[r];
      const float dot = sum16(y0 * dy0 + y1 * dy1);
      const float n = qn[il];
      const float dq0 = norm_bwd(dy0, y0, dot, n), dq1 = norm_bwd(dy1, y1, dot, n);
      if (i < N) {
        const int64_t row = token_row(d, b, i);
        if (row >= 0) {
          d.dqkv[row * C3 + g * HD + l15] = dq0;
          d.dqkv[row * C3 + g * HD + 16 + l15] = dq1;
        } else {
          pq0 += dq0;
          pq1 += dq1;
        }
      }
    }
  }
  // ---- per-workgroup partials: lane groups, then waves in a fixed order ----
  pq0 += __shfl_xor(pq0, 16);
  pq0 += __shfl_xor(pq0, 32);
  pq1 += __shfl_xor(pq1, 16);
  pq1 += __shfl_xor(pq1, 32);
  sacc = sum16(sacc);
  sacc += __shfl_xor(sacc, 16);
  sacc += __shfl_xor(sacc, 32);
  if (lg == 0) {
    red[wave * RQ + l15] = pq0;
    red[wave * RQ + 16 + l15] = pq1;
  }
  if (lane == 0) red[wave * RQ + HD] = sacc;
  __syncthreads();
  if (tid < RQ) P.ws_q[(int64_t)blockIdx.x * RQ + tid] = ((red[tid] + red[RQ + tid]) + red[2 * RQ + tid]) + red[3 * RQ + tid];
}

__global__ __launch_bounds__(256) void win_attn_large_ann_bwd_key_kernel(AnnBwdParams P) {
  __shared__ __attribute__((aligned(16))) float Ks[TB * LDW];      // k^ of this workgroup's keys
  __shared__ __attribute__((aligned(16))) float Vs[TB * LDW];      // v of them
  __shared__ __attribute__((aligned(16))) float Qs[TB * LDW];      // q^ of the current query block
  __shared__ __attribute__((aligned(16))) float Gs[TB * LDW];      // dO of it
  __shared__ float kn[TB];                                         // |k| of the keys
  __shared__ float rm[TB], rl[TB], rD[TB];                         // the block's row statistics
  __shared__ float red[4 * RK];
  const SdfWinAttnBwdDesc& d = P.d;
  const int N = d.N, NP = padded_n(N), G = groups_of(N);
  const int bg = blockIdx.x / G, kg = blockIdx.x - bg * G;
  const int b = bg / d.nH, g = bg - b * d.nH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int C = d.nH * HD;
  const int64_t C3 = 3 * (int64_t)C;
  const int k0 = kg * TB;
  const int kt0 = k0 + wave * 16;                        // first key of this wave's tile
  const bool active = kt0 < N;
  const int kj = kt0 + l15;                              // this lane's key (column of the S / dP blocks)

  stage_rows<1, true>(d, b, g, k0, Ks, kn, tid);
  stage_rows<2, false>(d, b, g, k0, Vs, nullptr, tid);
  __syncthreads();
  float kreg[8], vreg[8];
  load_row8(&Ks[(wave * 16 + l15) * LDW + 8 * lg], kreg);
  load_row8(&Vs[(wave * 16 + l15) * LDW + 8 * lg], vreg);

  const float ls = d.scale[g];
  const float* bias_g = d.bias + (int64_t)g * N * N;
  const float* mask_w = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
  const int nblk = groups_of(N);

  f32x4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = {0.f, 0.f, 0.f, 0.f}, dk0 = {0.f, 0.f, 0.f, 0.f}, dk1 = {0.f, 0.f, 0.f, 0.f};
  for (int blk = 0; blk < nblk; ++blk) {
    const int qb0 = blk * TB;
    __syncthreads();                                     // every wave is done with the previous block
    stage_rows<0, true>(d, b, g, qb0, Qs, nullptr, tid);
    stage_rows<3, false>(d, b, g, qb0, Gs, nullptr, tid);
    if (tid < TB) {
      const bool in = qb0 + tid < NP;                    // rows N .. NP - 1 were written by the query kernel; beyond NP: none
      const int64_t so = (int64_t)bg * NP + qb0 + tid;
      rm[tid] = in ? P.ws_m[so] : 0.f;
      rl[tid] = in ? P.ws_l[so] : 0.f;
      rD[tid] = in ? P.ws_D[so] : 0.f;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll
    for (int it = 0; it < TB / 16; ++it) {
      if (qb0 + it * 16 >= N) break;                     // (wave-uniform)
      const int qa = it * 16 + l15;                      // A operand row: query (inside the block)
      const f32x4 acc = mfma_row8(&Qs[qa * LDW + 8 * lg], kreg);
      const f32x4 dacc = mfma_row8(&Gs[qa * LDW + 8 * lg], vreg);
      // lane holds S / dP [query qb0 + 16 it + 4 lg + r][key kj]: P from the stored row statistics, dS
      float p[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = it * 16 + 4 * lg + r, i = qb0 + il;
        const bool ok = i < N && kj < N;
        const float bv = ok ? bias_g[(int64_t)i * N + kj] : 0.f;
        const float mv = (ok && mask_w) ? mask_w[(int64_t)i * N + kj] : 0.f;
        const float sc = attn_score(acc[r], ls, bv, mv, true, 0.f);
        p[r] = ok ? expf(sc - rm[il]) * rl[il] : 0.f;
        ds[r] = p[r] * (dacc[r] - rD[il]);
      }
      // dv += P^T dO, dk^ / scale += dS^T Q^ : A = the block (row key l15, k = query 4 lg + s), B = dO / q^[query][dim 16 dt + l15]
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int q = it * 16 + 4 * lg + s;
        dv0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], Gs[q * LDW + l15], dv0, 0, 0, 0);
        dv1 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], Gs[q * LDW + 16 + l15], dv1, 0, 0, 0);
        dk0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[s], Qs[q * LDW + l15], dk0, 0, 0, 0);
        dk1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[s], Qs[q * LDW + 16 + l15], dk1, 0, 0, 0);
      }
    }
  }

  // dv0[r] = dv[key kt0 + 4 lg + r][dim l15]; dk^ = scale dk; normalize backward; store
  float pk0 = 0.f, pk1 = 0.f, pv0 = 0.f, pv1 = 0.f;
  if (active) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jl = wave * 16 + 4 * lg + r, j = k0 + jl;
      const float y0 = Ks[jl * LDW + l15], y1 = Ks[jl * LDW + 16 + l15];
      const float dy0 = ls * dk0[r], dy1 = ls * dk1[r];
      const float dot = sum16(y0 * dy0 + y1 * dy1);
      const float n = kn[jl];
      const float dkx = norm_bwd(dy0, y0, dot, n), dky = norm_bwd(dy1, y1, dot, n);
      if (j < N) {
        const int64_t row = token_row(d, b, j);
        if (row >= 0) {
          float* o = d.dqkv + row * C3 + g * HD;
          o[C + l15] = dkx;
          o[C + 16 + l15] = dky;
          o[2 * C + l15] = dv0[r];
          o[2 * C + 16 + l15] = dv1[r];
        } else {
          pk0 += dkx;
          pk1 += dky;
          pv0 += dv0[r];
          pv1 += dv1[r];
        }
      }
    }
  }
  float part[4] = {pk0, pk1, pv0, pv1};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    part[i] += __shfl_xor(part[i], 16);
    part[i] += __shfl_xor(part[i], 32);
  }
  if (lg == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave * RK + 16 * i + l15] = part[i];
  }
  __syncthreads();
  if (tid < RK) P.ws_kv[(int64_t)blockIdx.x * RK + tid] = ((red[tid] + red[RK + tid]) + red[2 * RK + tid]) + red[3 * RK + tid];
}

// d_bias partial of one run of windows: the 64 x 64 tile (query group qg, key block kb) of head g.  grid (runs, nH, G * G).
__global__ __launch_bounds__(256) void win_attn_large_ann_bwd_dbias_kernel(AnnBwdParams P) {
  __shared__ __attribute__((aligned(16))) float Qs[TB * LDW];
  __shared__ __attribute__((aligned(16))) float Gs[TB * LDW];
  __shared__ __attribute__((aligned(16))) float Ks[TB * LDW];
  __shared__ __attribute__((aligned(16))) float Vs[TB * LDW];
  const SdfWinAttnBwdDesc& d = P.d;
  const int N = d.N, NP = padded_n(N), G = groups_of(N);
  const int run = blockIdx.x, g = blockIdx.y;
  const int qg = blockIdx.z / G, kb = blockIdx.z - qg * G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int q0 = qg * TB, kb0 = kb * TB;
  const int qt0 = q0 + wave * 16;
  const bool active = qt0 < N;
  const int qi = qt0 + l15;
  const float ls = d.scale[g];
  const float* bias_g = d.bias + (int64_t)g * N * N;
  const int b0 = run * P.wrun, b1 = min(d.B_, b0 + P.wrun);

  f32x4 acc[TB / 16];
#pragma unroll
  for (int jt = 0; jt < TB / 16; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b = b0; b < b1; ++b) {
    __syncthreads();                                     // the previous window is read out
    stage_rows<0, true>(d, b, g, q0, Qs, nullptr, tid);
    stage_rows<3, false>(d, b, g, q0, Gs, nullptr, tid);
    stage_rows<1, true>(d, b, g, kb0, Ks, nullptr, tid);
    stage_rows<2, false>(d, b, g, kb0, Vs, nullptr, tid);
    __syncthreads();
    if (!active) continue;
    float qreg[8], greg[8];
    load_row8(&Qs[(wave * 16 + l15) * LDW + 8 * lg], qreg);
    load_row8(&Gs[(wave * 16 + l15) * LDW + 8 * lg], greg);
    const float* mask_w = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
    const int64_t so = ((int64_t)b * d.nH + g) * NP + qi;          // qi < NP
    const float m = P.ws_m[so], inv = P.ws_l[so], Dq = P.ws_D[so];
    f32x4 st[TB / 16], dp[TB / 16];
    score_strip(Ks, Vs, qreg, greg, qi, kb0, N, ls, bias_g, mask_w, l15, lg, st, dp);
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[jt][r] += (expf(st[jt][r] - m) * inv) * (dp[jt][r] - Dq);
    }
  }
  if (active && qi < N) {
    float* p = P.ws_part + (((int64_t)run * d.nH + g) * N + qi) * N;
#pragma unroll
    for (int jt = 0; jt < TB / 16; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb0 + jt * 16 + 4 * lg + r;
        if (key < N) p[key] = acc[jt][r];
      }
    }
  }
}

// d_scale (nH) and d_pad (3C): the workgroups' partials in (window, group) order.  One thread per output element.
__global__ __launch_bounds__(256) void win_attn_large_ann_bwd_reduce_kernel(AnnBwdParams P) {
  const SdfWinAttnBwdDesc& d = P.d;
  const int nH = d.nH, C = nH * HD, G = groups_of(d.N);
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nH) {
    float s = 0.f;
    for (int w = 0; w < d.B_; ++w)
      for (int q = 0; q < G; ++q) s += P.ws_q[(((int64_t)w * nH + idx) * G + q) * RQ + HD];
    d.d_scale[idx] = s;
  } else if (idx < nH + 3 * C) {
    const int c = idx - nH;
    const int part = c / C, rest = c - part * C, g = rest / HD, dd = rest - g * HD;
    float s = 0.f;
    for (int w = 0; w < d.B_; ++w)
      for (int q = 0; q < G; ++q) {
        const int64_t wg = ((int64_t)w * nH + g) * G + q;
        s += part == 0 ? P.ws_q[wg * RQ + dd] : P.ws_kv[wg * RK + (part - 1) * HD + dd];
      }
    if (d.d_pad) d.d_pad[c] = s;
  }
}

// =====================================================================================================================================
// SEW
// =====================================================================================================================================
constexpr int LDO = HD + 1;           // padded fp32 row of dO (floats)
constexpr int LDG = HD + 4;           // Gram row (floats; float4 reads)
constexpr int LDK = TB + 1;           // padded row of a 64 x 64 (bias + mask) block
constexpr int RT = 16;                // query rows per d_bias workgroup
constexpr int KBD = 256;              // keys per d_bias workgroup (one per thread)
constexpr int LDV = HD + 4;           // fp32 row of V in the d_bias kernel (float4 reads)

__host__ __device__ inline int sew_dbias_tiles(int nH, int N) { return nH * ((N + RT - 1) / RT) * ((N + KBD - 1) / KBD); }

// tokens n0 .. n0 + 63 of one head's contiguous N x 32 byte block -> dst[64 * 32] (zeros past N)
__device__ __forceinline__ void stage_bytes(const uint8_t* head, int n0, int N, unsigned char* dst, int tid) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(head);
  uint32_t* D4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
  for (int i = tid; i < TB * HD / 4; i += 256) {
    const int w = n0 * (HD / 4) + i;
    D4[i] = w < N * (HD / 4) ? src[w] : 0u;
  }
}

// dO of tokens n0 .. n0 + 63 of (window b, head g) -> dst[64][LDO] (zeros past N)
__device__ __forceinline__ void stage_dout(const SdfWinAttnSewBwdDesc& d, int b, int g, int n0, int N, float* dst, int tid) {
#pragma unroll
  for (int i = tid; i < TB * (HD / 4); i += 256) {
    const int n = i >> 3, e4 = (i & 7) * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n0 + n < N) x = *reinterpret_cast<const float4*>(dout_row(d, b, g, n0 + n) + e4);
    float* r = dst + n * LDO + e4;
    r[0] = x.x;
    r[1] = x.y;
    r[2] = x.z;
    r[3] = x.w;
  }
}

__global__ __launch_bounds__(256) void win_attn_large_sew_bwd_gram_kernel(SdfWinAttnSewBwdDesc d, float* g3_out) {
  __shared__ __attribute__((aligned(16))) float dO[TB * LDO];                  // dO of the current token block
  __shared__ __attribute__((aligned(16))) float G1[HD * LDG];                  // V^T K
  __shared__ __attribute__((aligned(16))) float G3[HD * LDG];                  // Q^T dO
  __shared__ __attribute__((aligned(16))) unsigned char Qs[TB * HD];
  __shared__ __attribute__((aligned(16))) unsigned char Ks[TB * HD];
  __shared__ __attribute__((aligned(16))) unsigned char Vs[TB * HD];
  const int N = d.N1 * d.Tq, nH = d.nH;
  const int bg = blockIdx.x, b = bg / nH, g = bg - b * nH;
  const int tid = threadIdx.x;
  const int64_t head_off = (int64_t)bg * N * HD;                // raw head view: (b, g) is one contiguous N x 32 block
  const int r8 = tid >> 3, e0 = (tid & 7) * 4;                  // 32 rows x 8 column quads

  // ---- Grams: G1[r][e] = sum_n V[n][r] K[n][e],  G3[r][e] = sum_n Q[n][r] dO[n][e], n ascending ----
  {
    float a1[4] = {0.f, 0.f, 0.f, 0.f}, a3[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < N; n0 += TB) {
      __syncthreads();                                          // the previous block is read out
      stage_bytes(d.q + head_off, n0, N, Qs, tid);
      stage_bytes(d.k + head_off, n0, N, Ks, tid);
      stage_bytes(d.v + head_off, n0, N, Vs, tid);
      stage_dout(d, b, g, n0, N, dO, tid);
      __syncthreads();
      const int cnt = min(TB, N - n0);
      for (int n = 0; n < cnt; ++n) {
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
    }
    *reinterpret_cast<float4*>(G1 + r8 * LDG + e0) = make_float4(a1[0], a1[1], a1[2], a1[3]);
    *reinterpret_cast<float4*>(G3 + r8 * LDG + e0) = make_float4(a3[0], a3[1], a3[2], a3[3]);
  }

  const float sc = d.scale[g];
  // ---- dQ[n][e] = scale sum_r dO[n][r] G1[r][e];  dK[n][e] = scale sum_r V[n][r] G3[e][r] ----
  for (int n0 = 0; n0 < N; n0 += TB) {
    __syncthreads();                                            // the Grams are written / the previous block is read out
    stage_bytes(d.v + head_off, n0, N, Vs, tid);
    stage_dout(d, b, g, n0, N, dO, tid);
    __syncthreads();
    for (int nl = r8; nl < TB; nl += 32) {
      const int n = n0 + nl;
      if (n >= N) break;
      float aq[4] = {0.f, 0.f, 0.f, 0.f}, ak[4] = {0.f, 0.f, 0.f, 0.f};
      const float* o = dO + nl * LDO;
      const unsigned char* vrow = Vs + nl * HD;
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
  }

  // ---- Q^T dO goes to the workspace for the dV kernel ----
  *reinterpret_cast<float4*>(g3_out + (int64_t)bg * HD * HD + r8 * HD + e0) = *reinterpret_cast<const float4*>(G3 + r8 * LDG + e0);
}

// dV[m][e] = scale sum_r K[m][r] G3[r][e] + sum_n (bias + mask)[n][m] dO[n][e], n ascending.  Workgroup = (window, head, 64 keys): a thread
// owns keys r8 and 32 + r8 of the block and four dims; (bias + mask) and dO stream through LDS in 64-query blocks.
__global__ __launch_bounds__(256) void win_attn_large_sew_bwd_dv_kernel(SdfWinAttnSewBwdDesc d, const float* g3_in) {
  __shared__ __attribute__((aligned(16))) float dO[TB * LDO];                  // dO of the current query block
  __shared__ __attribute__((aligned(16))) float G3[HD * LDG];                  // Q^T dO
  __shared__ __attribute__((aligned(16))) float BM[TB * LDK];                  // bias + mask: 64 queries x 64 keys
  const int N = d.N1 * d.Tq, nH = d.nH, G = groups_of(N);
  const int bg = blockIdx.x / G, m0 = (blockIdx.x - bg * G) * TB;
  const int b = bg / nH, g = bg - b * nH;
  const int tid = threadIdx.x;
  const int64_t head_off = (int64_t)bg * N * HD;
  const int r8 = tid >> 3, e0 = (tid & 7) * 4;
  *reinterpret_cast<float4*>(G3 + r8 * LDG + e0) = *reinterpret_cast<const float4*>(g3_in + (int64_t)bg * HD * HD + r8 * HD + e0);
  __syncthreads();
  const float sc = d.scale[g];
  float ag[2][4], ab[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int m = m0 + r8 + 32 * h;
#pragma unroll
    for (int u = 0; u < 4; ++u) ag[h][u] = ab[h][u] = 0.f;
    if (m < N) {
      const uint32_t* krow = reinterpret_cast<const uint32_t*>(d.k + head_off + (int64_t)m * HD);
#pragma unroll
      for (int r4 = 0; r4 < HD / 4; ++r4) {
        const float4 kk = u8x4_f(krow[r4]);
        const float kf[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 g3 = *reinterpret_cast<const float4*>(G3 + (4 * r4 + u) * LDG + e0);
          ag[h][0] = fmaf(kf[u], g3.x, ag[h][0]);
          ag[h][1] = fmaf(kf[u], g3.y, ag[h][1]);
          ag[h][2] = fmaf(kf[u], g3.z, ag[h][2]);
          ag[h][3] = fmaf(kf[u], g3.w, ag[h][3]);
        }
      }
    }
  }
  const float* bias = d.bias + (int64_t)g * N * N;
  const float* mask = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
  for (int n0 = 0; n0 < N; n0 += TB) {
    __syncthreads();                                            // the previous block is read out
    for (int i = tid; i < TB * TB; i += 256) {
      const int nl = i / TB, j = i - nl * TB, n = n0 + nl, mm = m0 + j;
      float x = 0.f;
      if (n < N && mm < N) {
        x = bias[(int64_t)n * N + mm];
        if (mask) x += mask[(int64_t)n * N + mm];
      }
      BM[nl * LDK + j] = x;
    }
    stage_dout(d, b, g, n0, N, dO, tid);
    __syncthreads();
    const int cnt = min(TB, N - n0);
    for (int n = 0; n < cnt; ++n) {
      const float w0 = BM[n * LDK + r8], w1 = BM[n * LDK + 32 + r8];
      const float* o = dO + n * LDO + e0;
      const float o0 = o[0], o1 = o[1], o2 = o[2], o3 = o[3];
      ab[0][0] = fmaf(w0, o0, ab[0][0]);
      ab[0][1] = fmaf(w0, o1, ab[0][1]);
      ab[0][2] = fmaf(w0, o2, ab[0][2]);
      ab[0][3] = fmaf(w0, o3, ab[0][3]);
      ab[1][0] = fmaf(w1, o0, ab[1][0]);
      ab[1][1] = fmaf(w1, o1, ab[1][1]);
      ab[1][2] = fmaf(w1, o2, ab[1][2]);
      ab[1][3] = fmaf(w1, o3, ab[1][3]);
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int m = m0 + r8 + 32 * h;
    if (m < N) {
      const int64_t off = head_off + (int64_t)m * HD + e0;
      *reinterpret_cast<float4*>(d.dv + off) = make_float4(fmaf(sc, ag[h][0], ab[h][0]), fmaf(sc, ag[h][1], ab[h][1]),
                                                           fmaf(sc, ag[h][2], ab[h][2]), fmaf(sc, ag[h][3], ab[h][3]));
    }
  }
}

// d_bias partial of one run of windows: rows n0 .. n0 + RT - 1 of head g, keys kb0 .. kb0 + 255 (thread = key).
// grid (runs, nH, query tiles * key blocks).
__global__ __launch_bounds__(256) void win_attn_large_sew_dbias_kernel(SdfWinAttnSewBwdDesc d, float* part, int wrun) {
  __shared__ __attribute__((aligned(16))) float Vf[KBD * LDV];
  __shared__ __attribute__((aligned(16))) float Or[RT * HD];
  const int N = d.N1 * d.Tq, nH = d.nH;
  const int KBLK = (N + KBD - 1) / KBD;
  const int run = blockIdx.x, g = blockIdx.y;
  const int qt = blockIdx.z / KBLK, kb0 = (blockIdx.z - qt * KBLK) * KBD, n0 = qt * RT;
  const int tid = threadIdx.x;
  const int rows = min(RT, N - n0);
  const int m = kb0 + tid;
  const int b0 = run * wrun, b1 = min(d.B_, b0 + wrun);
  float acc[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) acc[i] = 0.f;
  for (int b = b0; b < b1; ++b) {
    __syncthreads();                                            // the previous window is read out
    const uint32_t* v4 = reinterpret_cast<const uint32_t*>(d.v + ((int64_t)b * nH + g) * N * HD);
    for (int i = tid; i < KBD * HD / 4; i += 256) {
      const int nl = i >> 3, e4 = (i & 7) * 4;
      const int w = kb0 * (HD / 4) + i;
      *reinterpret_cast<float4*>(Vf + nl * LDV + e4) = u8x4_f(w < N * (HD / 4) ? v4[w] : 0u);
    }
    for (int i = tid; i < RT * (HD / 4); i += 256) {
      const int r = i >> 3, e4 = (i & 7) * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < rows) x = *reinterpret_cast<const float4*>(dout_row(d, b, g, n0 + r) + e4);
      *reinterpret_cast<float4*>(Or + r * HD + e4) = x;
    }
    __syncthreads();
    if (m < N) {
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
  if (m < N) {
    float* p = part + (((int64_t)run * nH + g) * N + n0) * N + m;
    for (int r = 0; r < rows; ++r) p[(int64_t)r * N] = acc[r];
  }
}

bool range_ok(int64_t N) { return N > N_ABOVE && N <= N_MAX; }

}  // namespace

extern "C" int64_t sdf_win_attn_large_ann_bwd_workspace_bytes(int B_, int nH, int N) {
  if (B_ < 1 || nH < 1 || !range_ok(N)) return 0;
  const int64_t NP = padded_n(N), bh = (int64_t)B_ * nH, G = groups_of(N);
  const int64_t runs = dbias_runs(B_, (int)(nH * G * G));
  return 3 * align256(bh * NP * 4) + align256(bh * G * RQ * 4) + align256(bh * G * RK * 4) + align256(runs * nH * N * N * 4);
}

extern "C" int sdf_win_attn_large_ann_bwd(const SdfWinAttnBwdDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (!d->qkv || !d->dout || !d->scale || !d->bias || !d->dqkv || !d->d_scale || !d->d_bias || !d->workspace)
    return SDF_E_NULL;
  if (d->row_map && (!d->pad_qkv || !d->d_pad)) return SDF_E_NULL;       // windowing through the map: needs the pad row and its gradient
  if (d->hd != HD || d->B_ < 1 || d->nH < 1 || !range_ok(d->N)) return SDF_E_SHAPE;
  if (d->mask && (d->nW < 1 || d->B_ % d->nW)) return SDF_E_SHAPE;
  if (d->workspace_bytes < sdf_win_attn_large_ann_bwd_workspace_bytes(d->B_, d->nH, d->N)) return SDF_E_SHAPE;
  if (!sdf_aligned(d->qkv, 16) || !sdf_aligned(d->dout, 16) || !sdf_aligned(d->dqkv, 4) ||
      !sdf_aligned(d->workspace, 256) || (d->pad_qkv && !sdf_aligned(d->pad_qkv, 16)))
    return SDF_E_ALIGN;
  const int64_t NP = padded_n(d->N), bh = (int64_t)d->B_ * d->nH, G = groups_of(d->N);
  if (bh * G >= (1LL << 31) || d->nH > 65535 || G * G > 65535) return SDF_E_SHAPE;     // the grids below
  AnnBwdParams P;
  P.d = *d;
  if (!d->mask) P.d.nW = 1;
  const int tiles = (int)(d->nH * G * G);
  const int runs = dbias_runs(d->B_, tiles);
  P.wrun = dbias_run(d->B_, tiles);
  char* ws = reinterpret_cast<char*>(d->workspace);
  const int64_t stat = align256(bh * NP * 4);
  P.ws_m = reinterpret_cast<float*>(ws);
  P.ws_l = reinterpret_cast<float*>(ws + stat);
  P.ws_D = reinterpret_cast<float*>(ws + 2 * stat);
  P.ws_q = reinterpret_cast<float*>(ws + 3 * stat);
  P.ws_kv = reinterpret_cast<float*>(ws + 3 * stat + align256(bh * G * RQ * 4));
  P.ws_part = reinterpret_cast<float*>(ws + 3 * stat + align256(bh * G * RQ * 4) + align256(bh * G * RK * 4));
  hipStream_t s = sdf_stream(stream);
  SDF_LAUNCH(win_attn_large_ann_bwd_query_kernel, dim3((unsigned)(bh * G)), dim3(256), 0, s, P);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(win_attn_large_ann_bwd_key_kernel, dim3((unsigned)(bh * G)), dim3(256), 0, s, P);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(win_attn_large_ann_bwd_dbias_kernel, dim3((unsigned)runs, (unsigned)d->nH, (unsigned)(G * G)), dim3(256), 0, s, P);
  SDF_LAUNCH_CHECK();
  const int64_t nb = (int64_t)d->nH * d->N * d->N;
  SDF_LAUNCH(win_attn_large_bwd_sum_runs_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, P.ws_part, d->d_bias, nb, runs);
  SDF_LAUNCH_CHECK();
  const int total = d->nH + 3 * d->nH * HD;
  SDF_LAUNCH(win_attn_large_ann_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, P);
  SDF_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t sdf_win_attn_large_sew_bwd_workspace_bytes(int B_, int nH, int N) {
  if (B_ < 1 || nH < 1 || !range_ok(N)) return 0;
  return align256((int64_t)dbias_runs(B_, sew_dbias_tiles(nH, N)) * nH * N * N * 4) + align256((int64_t)B_ * nH * HD * HD * 4);
}

extern "C" int sdf_win_attn_large_sew_bwd(const SdfWinAttnSewBwdDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (!d->q || !d->k || !d->v || !d->dout || !d->scale || !d->bias || !d->dq || !d->dk || !d->dv || !d->d_bias || !d->workspace)
    return SDF_E_NULL;
  if (d->hd != HD || d->B_ < 1 || d->nH < 1 || d->Tq < 1 || d->N1 < 1 || !range_ok((int64_t)d->Tq * d->N1)) return SDF_E_SHAPE;
  if (d->mask && (d->nW < 1 || d->B_ % d->nW)) return SDF_E_SHAPE;
  const int N = d->Tq * d->N1;
  if (d->workspace_bytes < sdf_win_attn_large_sew_bwd_workspace_bytes(d->B_, d->nH, N)) return SDF_E_SHAPE;
  if (!sdf_aligned(d->q, 4) || !sdf_aligned(d->k, 4) || !sdf_aligned(d->v, 4) || !sdf_aligned(d->dout, 16) ||
      !sdf_aligned(d->dq, 16) || !sdf_aligned(d->dk, 16) || !sdf_aligned(d->dv, 16) || !sdf_aligned(d->workspace, 256))
    return SDF_E_ALIGN;
  const int zt = ((N + RT - 1) / RT) * ((N + KBD - 1) / KBD);
  const int64_t bh = (int64_t)d->B_ * d->nH;
  if (bh * groups_of(N) >= (1LL << 31) || d->nH > 65535) return SDF_E_SHAPE;             // the grids below
  SdfWinAttnSewBwdDesc P = *d;
  if (!d->mask) P.nW = 1;
  const int tiles = sew_dbias_tiles(d->nH, N);
  const int wrun = dbias_run(d->B_, tiles), runs = dbias_runs(d->B_, tiles);
  float* part = reinterpret_cast<float*>(d->workspace);                                  // (runs, nH, N, N): d_bias partials
  float* g3 = reinterpret_cast<float*>(reinterpret_cast<char*>(d->workspace) + align256((int64_t)runs * d->nH * N * N * 4));   // (B_, nH, 32, 32)
  hipStream_t s = sdf_stream(stream);
  SDF_LAUNCH(win_attn_large_sew_bwd_gram_kernel, dim3((unsigned)bh), dim3(256), 0, s, P, g3);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(win_attn_large_sew_bwd_dv_kernel, dim3((unsigned)(bh * groups_of(N))), dim3(256), 0, s, P, (const float*)g3);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(win_attn_large_sew_dbias_kernel, dim3((unsigned)runs, (unsigned)d->nH, (unsigned)zt), dim3(256), 0, s, P, part, wrun);
  SDF_LAUNCH_CHECK();
  const int64_t nb = (int64_t)d->nH * N * N;
  SDF_LAUNCH(win_attn_large_bwd_sum_runs_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, part, d->d_bias, nb, runs);
  SDF_LAUNCH_CHECK();
  return 0;
}
