// Fused 3-D window attention for windows of 193 .. 1024 tokens (up to (2,22,22)): the arithmetic of win_attn.hip's win_attn_kernel -
// both modes, exact-fp32 MFMA for both products, S^T = K Q^T so that a key tile's accumulator is the A operand of P.V - with the
// keys walked in blocks instead of a whole 16 x N score strip in registers.
//
// One workgroup = (window, head, 64 queries): each of its four waves owns ONE 16-query tile and keeps, across the whole key walk,
// only the tile's two output accumulators, and in the ANN mode the running row maximum and row sum (online softmax: when a block
// raises a row's maximum, the row's sum and output accumulators are scaled by exp(old - new) first).  A block is KB = 64 keys: its K rows
// (L2-normalised on the way in for the ANN mode) and V^T are staged in 17.5 KiB of LDS by all four waves, the next block's rows are
// already in flight in registers while the current one is multiplied.  The same form serves every N of the range: nothing of the
// LDS or register budget depends on N, many workgroups share a compute unit, and no opt-in above 64 KiB is needed.
//
// A key past N scores -inf before the maximum (ANN) or 0 (SEW) and its K / V rows are zero.  Every block holds at least one real
// key and bias and mask are finite, so a block's row maximum is finite; how the running sum moves from one rounded reference point
// to the next, the first block and a block masked to -inf are win_attn_common.h's softmax_ref_step.
// No atomics: every output element has one writer and a fixed summation order.
// The query fragment, the K / V piece fetch and their F.normalize, the MFMA chain over an LDS row, the score rounding and the output
// offset are win_attn_common.h's too.
#include "win_attn_common.h"
#include "host_launch.h"

namespace {

constexpr int N_ABOVE = 192, N_MAX = 1024;   // served: N_ABOVE < N <= N_MAX (up to N_ABOVE: sdf_win_attn_fwd)
constexpr int KB = 64;                       // keys per staged block
constexpr int KT = KB / 16;                  // key tiles per block
constexpr int LDT = KB + 4;                  // padded V^T row (floats)

template <int MODE, bool HAS_MASK>
__global__ __launch_bounds__(256) void win_attn_large_kernel(AttnParams P) {
  __shared__ __attribute__((aligned(16))) float Ks[KB * LDW];      // [key][dim]
  __shared__ __attribute__((aligned(16))) float Vt[HD * LDT];      // [dim][key]
  const SdfWinAttnDesc& d = P.d;
  const int N = d.N, NT = (N + 15) / 16, QG = (NT + 3) / 4;

  const int bg = blockIdx.x / QG, qg = blockIdx.x - bg * QG;
  const int b = bg / d.nH, g = bg - b * d.nH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int C = d.nH * HD;
  const int qt = qg * 4 + wave;
  const bool active = qt * 16 < N;                       // (a wave without a query tile still stages keys and meets the barriers)
  const int qi = qt * 16 + l15;                          // this lane's query

  // ---- B operand of S^T = K Q^T: Q[qi][8 lg .. 8 lg + 7], normalised (ANN) / scaled (SEW: q * scale) ----
  float qreg[8];
  load_q_frag<MODE>(d, b, g, qi, lg, N, C, d.scale[g], qreg);
  if (MODE == SDF_ATTN_ANN) norm_q_frag(qreg);

  // ---- a key block's K and V rows: 8 lanes per token row (one float4 each), 32 rows per pass ----
  constexpr int IT = KB / 32;
  const int piece = tid & 7;
  float4 kq[IT], vq[IT];
  auto fetch = [&](int kb0) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = kb0 + (tid >> 3) + 32 * it;
      kq[it] = vq[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < N) kv_piece<MODE>(d, b, g, r, piece, C, kq[it], vq[it]);
    }
  };
  auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int r = (tid >> 3) + 32 * it;                // row inside the block
      float4 kv = kq[it];
      if (MODE == SDF_ATTN_ANN) norm_row8(kv);           // F.normalize(k, dim=-1)
      *reinterpret_cast<float4*>(&Ks[r * LDW + 4 * piece]) = kv;
      Vt[(4 * piece + 0) * LDT + r] = vq[it].x;
      Vt[(4 * piece + 1) * LDT + r] = vq[it].y;
      Vt[(4 * piece + 2) * LDT + r] = vq[it].z;
      Vt[(4 * piece + 3) * LDT + r] = vq[it].w;
    }
  };

  const float ls = (MODE == SDF_ATTN_ANN) ? d.scale[g] : 1.f;
  // bias / mask rows are only 4-byte aligned for odd N: one dword per load, a key or query past N as an out-of-range offset (zeros)
  const uint32_t tbytes = (uint32_t)N * (uint32_t)N * 4u;
  const __amdgpu_buffer_rsrc_t bias_rs = make_rsrc_bounded(d.bias + (int64_t)g * N * N, tbytes);
  const __amdgpu_buffer_rsrc_t mask_rs = make_rsrc_bounded(HAS_MASK ? d.mask + (int64_t)(b % d.nW) * N * N : d.bias, HAS_MASK ? tbytes : 0u);
  const uint32_t rowoff = (uint32_t)qi * (uint32_t)N * 4u;

  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;                  // ANN: running maximum and sum of this lane's query row
  float r_run = 0.f;                                     // ... and the reference point -m log2e the sum's terms were made with

  const int nblk = (N + KB - 1) / KB;
  fetch(0);
  for (int blk = 0; blk < nblk; ++blk) {
    const int kb0 = blk * KB;
    if (blk) __syncthreads();                            // every wave is done with the previous block
    stash();
    __syncthreads();
    if (blk + 1 < nblk) fetch(kb0 + KB);                 // in flight under this block's products
    if (!active) continue;

    // ---- request bias / mask of the 16 x KB strip ahead of the K Q^T products: lane needs [qi][kb0 + 16 jt + 4 lg + r] ----
    uint32_t bb[KT][4], mm[KT][4];
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kb0 + jt * 16 + 4 * lg + r;
        const uint32_t off = (qi < N && key < N) ? rowoff + (uint32_t)key * 4u : INV;
        bb[jt][r] = __builtin_amdgcn_raw_buffer_load_b32(bias_rs, off, 0, 0);
        mm[jt][r] = HAS_MASK ? __builtin_amdgcn_raw_buffer_load_b32(mask_rs, off, 0, 0) : 0u;
      }
    }
    // ---- S^T = K Q^T ----
    f32x4 st[KT];
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
      st[jt] = mfma_row8(&Ks[(jt * 16 + l15) * LDW + 8 * lg], qreg);   // A operand row: key (inside the block)
    }
    // ---- the scores (win_attn_common.h attn_score); a key past N: -inf / 0 ----
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        st[jt][r] = attn_score<HAS_MASK>(st[jt][r], ls, bb[jt][r], mm[jt][r], kb0 + jt * 16 + 4 * lg + r < N, key_past_n<MODE>());
    }
    if (MODE == SDF_ATTN_ANN) {
      float bm = st[0][0];
#pragma unroll
      for (int jt = 0; jt < KT; ++jt) bm = fmaxf(fmaxf(fmaxf(bm, st[jt][0]), fmaxf(st[jt][1], st[jt][2])), st[jt][3]);
      bm = fmaxf(bm, __shfl_xor(bm, 16));
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      float mneg, alpha;                                 // the new reference point, the old terms' factor (win_attn_common.h)
      const float m_new = softmax_ref_step(m_run, r_run, bm, mneg, alpha);
      float psum = 0.f;
#pragma unroll
      for (int jt = 0; jt < KT; ++jt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(fmaf(st[jt][r], L2E, mneg));
          st[jt][r] = e;
          psum += e;
        }
      }
      psum += __shfl_xor(psum, 16);
      psum += __shfl_xor(psum, 32);
      l_run = l_run * alpha + psum;
      m_run = m_new;
      r_run = mneg;
      if (__any(alpha != 1.f)) {                         // a maximum moved: the lane's four OUTPUT rows are queries 4 lg + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ar = __shfl(alpha, (lane & 48) | (4 * lg + r));
          o0[r] *= ar;
          o1[r] *= ar;
        }
      }
    }
    // ---- O += P V : A = P (registers), B = Vt[d = 16 dt + l15][key = 16 jt + 4 lg + s] ----
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
      const float4 v0 = *reinterpret_cast<const float4*>(&Vt[l15 * LDT + jt * 16 + 4 * lg]);
      const float4 v1 = *reinterpret_cast<const float4*>(&Vt[(16 + l15) * LDT + jt * 16 + 4 * lg]);
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][0], v0.x, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][0], v1.x, o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][1], v0.y, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][1], v1.y, o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][2], v0.z, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][2], v1.z, o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][3], v0.w, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][3], v1.w, o1, 0, 0, 0);
    }
  }
  if (!active) return;

  // ---- store: o[r] is query qt*16 + 4*lg + r, dim l15 (o0) / 16 + l15 (o1); ANN: divided by the row's sum ----
  const float inv = (MODE == SDF_ATTN_ANN) ? 1.f / l_run : 1.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float rinv = (MODE == SDF_ATTN_ANN) ? __shfl(inv, (lane & 48) | (4 * lg + r)) : 1.f;
    const int i = qt * 16 + 4 * lg + r;
    if (i < N) {
      int64_t off;
      if (!out_offset<MODE>(d, b, g, i, C, off)) continue;                   // a padding token
      d.out[off + l15] = o0[r] * rinv;
      d.out[off + 16 + l15] = o1[r] * rinv;
    }
  }
}

}  // namespace

extern "C" int sdf_win_attn_large_fwd(const SdfWinAttnDesc* d, void* stream) {
  if (const int rc = sdf_win_attn_desc_rc(d, N_ABOVE + 1, N_MAX)) return rc;
  const int64_t wgs = sdf_win_attn_group_grid(d);
  if (!wgs) return SDF_E_SHAPE;
  const AttnParams P = sdf_win_attn_params(d);
  const dim3 grid((unsigned)wgs), block(256);
  hipStream_t s = sdf_stream(stream);
  sdf_dispatch(SdfList<SDF_ATTN_ANN, SDF_ATTN_SEW>{}, d->mode, [&](auto mode) {
    if (d->mask) {
      SDF_LAUNCH((win_attn_large_kernel<mode, true>), grid, block, 0, s, P);
    } else {
      SDF_LAUNCH((win_attn_large_kernel<mode, false>), grid, block, 0, s, P);
    }
  });
  return sdf_launch_rc();
}
