// The attention MAP of the 3-D window attention, (B_, nH, N, N) fp32, for 1 <= N <= 1024 tokens per window: what the reference's
// attention modules return as their second value (`return_attention=True`, `log=True`).  The forward kernels (win_attn.hip,
// win_attn_large.hip) keep that matrix in registers and never store it; this kernel makes it alone, from the same operands with the
// same arithmetic - exact-fp32 MFMA products, the score rounded as (acc * scale[g] + bias) + mask - and touches no V and no output
// buffer.  ANN: the softmax probabilities of the cosine scores.  SEW: the scores themselves, acc = the exact integer count of
// common spikes of a query and a key.
//
// One workgroup = (window, head, 64 queries), as win_attn_large_kernel: each of its four waves owns ONE 16-query tile, the keys are
// walked in blocks of KB = 64 whose K rows (L2-normalised on the way in for the ANN mode) all four waves stage in 9 KiB of LDS,
// the next block's rows in flight in registers under the current block's products.  Nothing of the LDS or register budget depends
// on N.  Here S = Q K^T (the query tile is the A operand), so a lane's accumulator element r is (query 4 lg + r, key l15): a
// store instruction writes 16 consecutive keys of four rows, one dword per lane (rows are only 4-byte aligned at odd N).
//
// ANN walks the keys twice and takes no workspace: the first walk keeps each row's running maximum and sum (online softmax, the
// reference point handling of win_attn_large_kernel), the second recomputes every tile - the same loads, the same instructions, so
// the same bits - and stores exp(s - max) / sum.  SEW walks once and stores the score.
// A key or query at or past N contributes nothing (a key: -inf before the maximum, no term in the sum) and is never stored.
// No atomics: every element has one writer and every row sum one order, two calls give bit-equal results.
// The query fragment, the K piece fetch and their F.normalize, the MFMA chain (the row as B operand: mfma_row8_b), the score rounding
// and the reference-point step of the online softmax are win_attn_common.h's.
#include "win_attn_common.h"
#include "host_launch.h"

namespace {

constexpr int N_MAX = 1024;
constexpr int KB = 64;                       // keys per staged block
constexpr int KT = KB / 16;                  // key tiles per block

template <int MODE, bool HAS_MASK>
__global__ __launch_bounds__(256) void win_attn_scores_kernel(AttnParams P, float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float Ks[KB * LDW];      // [key][dim]
  const SdfWinAttnDesc& d = P.d;
  const int N = d.N, NT = (N + 15) / 16, QG = (NT + 3) / 4;

  const int bg = blockIdx.x / QG, qg = blockIdx.x - bg * QG;
  const int b = bg / d.nH, g = bg - b * d.nH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int C = d.nH * HD;
  const int qt = qg * 4 + wave;
  const bool active = qt * 16 < N;                       // (a wave without a query tile still stages keys and meets the barriers)
  const int qi = qt * 16 + l15;                          // the query this lane LOADS (A operand row)
  const int q0 = qt * 16 + 4 * lg;                       // the first of the four queries this lane's accumulators belong to

  // ---- A operand of S = Q K^T: Q[qi][8 lg .. 8 lg + 7], normalised (ANN) / the spikes as 0 or 1 (SEW) ----
  float qreg[8];
  load_q_frag<MODE>(d, b, g, qi, lg, N, C, 1.f, qreg);
  if (MODE == SDF_ATTN_ANN) norm_q_frag(qreg);

  // ---- a key block's K rows: 8 lanes per token row (one float4 each), 32 rows per pass ----
  constexpr int IT = KB / 32;
  const int piece = tid & 7;
  float4 kq[IT];
  auto fetch = [&](int kb0) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = kb0 + (tid >> 3) + 32 * it;
      kq[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 unused;                                     // (no V here)
      if (r < N) kv_piece<MODE, false>(d, b, g, r, piece, C, kq[it], unused);
    }
  };
  auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = (tid >> 3) + 32 * it;                // row inside the block
      float4 kv = kq[it];
      if (MODE == SDF_ATTN_ANN) norm_row8(kv);           // F.normalize(k, dim=-1)
      *reinterpret_cast<float4*>(&Ks[r * LDW + 4 * piece]) = kv;
    }
  };

  const float ls = d.scale[g];
  // bias / mask rows are only 4-byte aligned for odd N: one dword per load, a key or query past N as an out-of-range offset (zeros)
  const uint32_t tbytes = (uint32_t)N * (uint32_t)N * 4u;
  const __amdgpu_buffer_rsrc_t bias_rs = make_rsrc_bounded(d.bias + (int64_t)g * N * N, tbytes);
  const __amdgpu_buffer_rsrc_t mask_rs = make_rsrc_bounded(HAS_MASK ? d.mask + (int64_t)(b % d.nW) * N * N : d.bias, HAS_MASK ? tbytes : 0u);
  float* const tile = scores + (int64_t)bg * N * N;      // this (window, head)'s N x N map

  // ANN, per accumulator row r (query q0 + r): running maximum, sum, and the reference point -m log2e the sum's terms were made with
  float m_run[4], l_run[4], r_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; r_run[r] = 0.f; }

  const int nblk = (N + KB - 1) / KB;
  const int nstep = (MODE == SDF_ATTN_ANN) ? 2 * nblk : nblk;      // ANN: the walk for the row statistics, then the walk that stores
  fetch(0);
  for (int step = 0; step < nstep; ++step) {
    const bool second = step >= nblk;
    const int kb0 = (second ? step - nblk : step) * KB;
    if (step) __syncthreads();                           // every wave is done with the previous block
    stash();
    __syncthreads();
    if (step + 1 < nstep) fetch(step + 1 == nblk ? 0 : kb0 + KB);   // in flight under this block's products
    if (!active) continue;

    // ---- request bias / mask of the 16 x KB strip ahead of the products: lane needs [q0 + r][kb0 + 16 jt + l15] ----
    uint32_t bb[KT][4], mm[KT][4];
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
      const int key = kb0 + jt * 16 + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t off = (q0 + r < N && key < N) ? ((uint32_t)(q0 + r) * (uint32_t)N + (uint32_t)key) * 4u : INV;
        bb[jt][r] = __builtin_amdgcn_raw_buffer_load_b32(bias_rs, off, 0, 0);
        mm[jt][r] = HAS_MASK ? __builtin_amdgcn_raw_buffer_load_b32(mask_rs, off, 0, 0) : 0u;
      }
    }
    // ---- S = Q K^T ----
    f32x4 st[KT];
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
      st[jt] = mfma_row8_b(qreg, &Ks[(jt * 16 + l15) * LDW + 8 * lg]);   // B operand column: key (inside the block)
    }
    // ---- attn = qk * scale + bias (+ mask), separately rounded as the reference computes it; ANN: a key past N is -inf ----
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
      const bool kin = kb0 + jt * 16 + l15 < N;
#pragma unroll
      for (int r = 0; r < 4; ++r) st[jt][r] = attn_score<HAS_MASK>(st[jt][r], ls, bb[jt][r], mm[jt][r], MODE != SDF_ATTN_ANN || kin, -INFINITY);
    }
    if (MODE == SDF_ATTN_ANN && !second) {
      // every block holds at least one real key and bias and mask are finite, so a block's row maximum is finite (a caller's mask
      // of -inf over a whole block is met with a zero reference point, as in win_attn_large_kernel)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float bm = fmaxf(fmaxf(st[0][r], st[1][r]), fmaxf(st[2][r], st[3][r]));
        bm = fmaxf(bm, __shfl_xor(bm, 1));
        bm = fmaxf(bm, __shfl_xor(bm, 2));
        bm = fmaxf(bm, __shfl_xor(bm, 4));
        bm = fmaxf(bm, __shfl_xor(bm, 8));
        float mneg, alpha;                               // the new reference point, the old terms' factor (win_attn_common.h)
        const float m_new = softmax_ref_step(m_run[r], r_run[r], bm, mneg, alpha);
        float psum = 0.f;
#pragma unroll
        for (int jt = 0; jt < KT; ++jt) psum += __builtin_amdgcn_exp2f(fmaf(st[jt][r], L2E, mneg));
        psum += __shfl_xor(psum, 1);
        psum += __shfl_xor(psum, 2);
        psum += __shfl_xor(psum, 4);
        psum += __shfl_xor(psum, 8);
        l_run[r] = l_run[r] * alpha + psum;
        m_run[r] = m_new;
        r_run[r] = mneg;
      }
      continue;
    }
    // ---- store: st[jt][r] is (query q0 + r, key kb0 + 16 jt + l15); ANN: exp(s - max) / sum ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (q0 + r >= N) continue;
      const float inv = (MODE == SDF_ATTN_ANN) ? 1.f / l_run[r] : 1.f;
      float* const row = tile + (int64_t)(q0 + r) * N;
#pragma unroll
      for (int jt = 0; jt < KT; ++jt) {
        const int key = kb0 + jt * 16 + l15;
        if (key >= N) continue;
        row[key] = (MODE == SDF_ATTN_ANN) ? __builtin_amdgcn_exp2f(fmaf(st[jt][r], L2E, r_run[r])) * inv : st[jt][r];
      }
    }
  }
}

}  // namespace

extern "C" int sdf_win_attn_scores_fwd(const SdfWinAttnDesc* d, float* scores, void* stream) {
  if (!d) return SDF_E_NULL;
  if (!d->q || (d->mode == SDF_ATTN_SEW && !d->k) || !d->scale || !d->bias || (d->row_map && !d->pad_qkv)) return SDF_E_NULL;
  if (const int rc = sdf_win_attn_shape_rc(d, 1, N_MAX)) return rc;
  if (d->mode == SDF_ATTN_SEW && d->row_map) return SDF_E_SHAPE;    // windowing through the map is the ANN form
  if (!scores) return SDF_E_NULL;
  if (!sdf_aligned(scores, 4)) return SDF_E_ALIGN;
  if (!sdf_aligned(d->q, d->mode == SDF_ATTN_ANN ? 16 : 4)) return SDF_E_ALIGN;                    // float4 rows / 4 spikes per load
  if (d->mode == SDF_ATTN_SEW ? !sdf_aligned(d->k, 4) : (d->row_map && !sdf_aligned(d->pad_qkv, 16))) return SDF_E_ALIGN;
  const int64_t wgs = sdf_win_attn_group_grid(d);
  if (!wgs) return SDF_E_SHAPE;
  const AttnParams P = sdf_win_attn_params(d);
  const dim3 grid((unsigned)wgs), block(256);
  hipStream_t s = sdf_stream(stream);
  sdf_dispatch(SdfList<SDF_ATTN_ANN, SDF_ATTN_SEW>{}, d->mode, [&](auto mode) {
    if (d->mask) {
      SDF_LAUNCH((win_attn_scores_kernel<mode, true>), grid, block, 0, s, P, scores);
    } else {
      SDF_LAUNCH((win_attn_scores_kernel<mode, false>), grid, block, 0, s, P, scores);
    }
  });
  return sdf_launch_rc();
}
