// What the six window-attention files share, each stated once (win_attn.hip, win_attn_large.hip, win_attn_scores.hip, win_attn_bwd.hip,
// win_attn_sew_bwd.hip, win_attn_large_bwd.hip): the constants, the spike unpack, the query fragment and the 8-lanes-per-row K / V piece
// with their F.normalize, the eight-step exact-fp32 MFMA chain over one LDS row in both operand orders, the score rounding, the
// online-softmax reference point, the output offset of a token, the backward's helpers, and - host code only, at the end - the desc
// checks and the launch preamble of the three forward entry points.  A kernel file shows what is its own: walk order, LDS layout,
// pipelining.
// Every function is always_inline and takes the values the sites hold (N, C as arguments, not re-read from the desc).  No kernel's
// registers, spills, scratch, occupancy or LDS moved; 16 kernels are identical to what they were with the text written out, 23 are
// scheduled differently, bit-equal and as fast (profiles/win_attn_shared_device_code.txt).  Two sites keep their text because a
// function moved a VGPR count: win_attn_tiled_kernel's load_q, and pass 1 of win_attn_ann_bwd_kernel as a call of score_strip.
#pragma once
#include "device_prims.h"

namespace {

constexpr int HD = 32;
constexpr int LDW = HD + 4;                     // padded LDS row (floats)
constexpr float NEPS = 1e-12f;                  // F.normalize eps
constexpr float L2E = 1.4426950408889634f;      // log2(e): exp(x - m) = 2^(x log2e - m log2e), one fma + the hardware exp2

struct AttnParams {
  SdfWinAttnDesc d;
};

__host__ __device__ inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
__host__ __device__ inline int padded_n(int N) { return ((N + 15) / 16) * 16; }

// ---- tokens and rows ----------------------------------------------------------------------------------------------------------------
// row of token r of window b in the (rows, 3C) / (rows, C) buffers, or -1 for a padding token (forward and backward desc alike)
template <class Desc>
__device__ __forceinline__ int64_t token_row(const Desc& d, int b, int r) {
  return d.row_map ? (int64_t)d.row_map[(int64_t)b * d.N + r] : (int64_t)b * d.N + r;
}

// ANN mode: first float of the q | k | v row of token r of window b.  With a row map the window partition (pad, roll, reshape)
// is this lookup; a padding token reads the qkv Linear's image of a zero row.
__device__ __forceinline__ const float* qkv_row(const SdfWinAttnDesc& d, int b, int r, int C) {
  const float* q = reinterpret_cast<const float*>(d.q);
  if (!d.row_map) return q + ((int64_t)b * d.N + r) * 3 * C;
  const int row = d.row_map[(int64_t)b * d.N + r];
  return row >= 0 ? q + (int64_t)row * 3 * C : d.pad_qkv;
}

// SEW mode: row of token i of window b in the (T', B_, N1, C) layout the output leaves through: (B_,nH,T',N1,hd) -> (T',B_,N1,C)
template <class I>
__device__ __forceinline__ I sew_row(int i, int b, int B_, int N1) {
  const int t = i / N1, n1 = i - t * N1;
  return ((I)t * B_ + b) * N1 + n1;
}

// Offset in `out` of dim 0 of head g of token i of window b; false for an ANN padding token: no store (the reference crops it away).
// ANN: (attn @ v).transpose(1, 2).reshape(B_, N, C) [+ window reverse + roll back + crop through the row map]
template <int MODE>
__device__ __forceinline__ bool out_offset(const SdfWinAttnDesc& d, int b, int g, int i, int C, int64_t& off) {
  if (MODE == SDF_ATTN_ANN) {
    const int64_t orow = token_row(d, b, i);
    if (orow < 0) return false;
    off = orow * C + g * HD;
  } else {
    off = sew_row<int64_t>(i, b, d.B_, d.N1) * C + g * HD;
  }
  return true;
}

// dO row n of window b, head g in the SEW backward's scrambled (T', B_, N1, C) layout
__device__ inline const float* dout_row(const SdfWinAttnSewBwdDesc& d, int b, int g, int n) {
  return d.dout + sew_row<int64_t>(n, b, d.B_, d.N1) * (int64_t)(d.nH * HD) + g * HD;
}

// ---- operand loads ------------------------------------------------------------------------------------------------------------------
// four byte spikes -> their values / -> `on` where a spike is set
__device__ inline float4 u8x4_f(uint32_t w) {
  return make_float4((float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu), (float)(w >> 24));
}
__device__ __forceinline__ float4 u8x4_on(uint32_t w, const float& on) {
  return make_float4((w & 0xffu) ? on : 0.f, ((w >> 8) & 0xffu) ? on : 0.f, ((w >> 16) & 0xffu) ? on : 0.f, (w >> 24) ? on : 0.f);
}

// eight consecutive floats (two float4) of a row
__device__ __forceinline__ void load_row8(const float* row, float (&o)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(row);
  const float4 c = *reinterpret_cast<const float4*>(row + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = c.x; o[5] = c.y; o[6] = c.z; o[7] = c.w;
}

// Q fragment of query qi for lane group lg: Q[qi][8 lg .. 8 lg + 7], zeros past N.  SEW: a set spike becomes `on` (scale[g]: q * scale
// of the reference; 1.f where the scale multiplies the exact count afterwards).  N and C = nH * HD are the site's values.
template <int MODE>
__device__ __forceinline__ void load_q_frag(const SdfWinAttnDesc& d, int b, int g, int qi, int lg, int N, int C, float on, float (&qr)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) qr[i] = 0.f;
  if (qi < N) {
    if (MODE == SDF_ATTN_ANN) {
      load_row8(qkv_row(d, b, qi, C) + g * HD + 8 * lg, qr);
    } else {
      const uint8_t* qp = reinterpret_cast<const uint8_t*>(d.q) + (((int64_t)b * d.nH + g) * N + qi) * HD + 8 * lg;
      const uint32_t w0 = *reinterpret_cast<const uint32_t*>(qp), w1 = *reinterpret_cast<const uint32_t*>(qp + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qr[i] = ((w0 >> (8 * i)) & 0xff) ? on : 0.f;
        qr[4 + i] = ((w1 >> (8 * i)) & 0xff) ? on : 0.f;
      }
    }
  }
}
// max(||q||_2, eps) of the fragment's row; its four lane groups are lanes 16 and 32 apart
__device__ __forceinline__ float q_frag_norm(const float (&qr)[8]) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss += qr[i] * qr[i];
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);
  return fmaxf(sqrtf(ss), NEPS);
}
// F.normalize(q, dim=-1) of the fragment: x / max(||x||_2, eps)
__device__ __forceinline__ void norm_q_frag(float (&qr)[8]) {
  const float iq = 1.f / q_frag_norm(qr);
#pragma unroll
  for (int i = 0; i < 8; ++i) qr[i] *= iq;
}

// K and (WITH_V) V of token r < N, head g: the four dims 4 piece .. 4 piece + 3 - 8 lanes per token row, one float4 each, whole
// 128-byte lines per request.  The map kernel takes K alone (v is left as it is, d.v is not read).
template <int MODE, bool WITH_V = true>
__device__ __forceinline__ void kv_piece(const SdfWinAttnDesc& d, int b, int g, int r, int piece, int C, float4& k, float4& v) {
  if (MODE == SDF_ATTN_ANN) {
    const float* base = qkv_row(d, b, r, C) + g * HD + 4 * piece;
    k = *reinterpret_cast<const float4*>(base + C);
    if (WITH_V) v = *reinterpret_cast<const float4*>(base + 2 * C);
  } else {
    const int64_t off = (((int64_t)b * d.nH + g) * d.N + r) * HD + 4 * piece;
    const uint32_t wk = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(d.k) + off);
    const uint32_t wv = WITH_V ? *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(d.v) + off) : 0u;
    k = u8x4_f(wk);
    if (WITH_V) v = u8x4_f(wv);
  }
}
// F.normalize of a row held as 8 pieces by 8 neighbouring lanes; returns the raw norm for the callers that keep it
__device__ __forceinline__ float norm_row8(float4& x) {
  float ss = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  ss += __shfl_xor(ss, 4);
  const float n = sqrtf(ss), inv = 1.f / fmaxf(n, NEPS);
  x.x *= inv; x.y *= inv; x.z *= inv; x.w *= inv;
  return n;
}

// ---- products -----------------------------------------------------------------------------------------------------------------------
// eight k-steps of the exact 16 x 16 x 4 fp32 MFMA (a k-ordered fmaf chain) over this lane's LDS row (dims 8 lg .. 8 lg + 7) against
// a register fragment.  mfma_row8: the row is the A operand (S^T = K Q^T: a key tile's accumulator is the A operand of P V);
// mfma_row8_b: the row is the B operand (S = Q K^T: the accumulator element r is (query 4 lg + r, key l15)).
__device__ __forceinline__ f32x4 mfma_row8(const float* arow, const float (&b)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(arow);
  const float4 c = *reinterpret_cast<const float4*>(arow + 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c.x, b[4], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c.y, b[5], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c.z, b[6], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c.w, b[7], acc, 0, 0, 0);
  return acc;
}

__device__ __forceinline__ f32x4 mfma_row8_b(const float (&a)[8], const float* brow) {
  const float4 b = *reinterpret_cast<const float4*>(brow);
  const float4 c = *reinterpret_cast<const float4*>(brow + 4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b.w, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4], c.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[5], c.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[6], c.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[7], c.w, acc, 0, 0, 0);
  return acc;
}

// ---- scores -------------------------------------------------------------------------------------------------------------------------
// what a key past N scores: -inf before the maximum (ANN: P = 0), 0 (SEW)
template <int MODE>
__device__ __forceinline__ constexpr float key_past_n() {
  return MODE == SDF_ATTN_ANN ? -INFINITY : 0.f;
}
// attn = qk * logit_scale + bias (+ mask): separately rounded, as the reference computes it; `past` where the key is not in range
template <bool HAS_MASK = true>
__device__ __forceinline__ float attn_score(float acc, float ls, float bv, float mv, bool in, float past) {
  float s = acc * ls + bv;
  if (HAS_MASK) s += mv;
  return in ? s : past;
}
// the same on the words of a buffer load
template <bool HAS_MASK>
__device__ __forceinline__ float attn_score(float acc, float ls, uint32_t bw, uint32_t mw, bool in, float past) {
  return attn_score<HAS_MASK>(acc, ls, __uint_as_float(bw), __uint_as_float(mw), in, past);
}
// ... and on the four keys kb .. kb + 3 a lane holds of one key tile, bias and mask as the words of one 16-byte load each (the
// tiled kernels); `ragged`: the tile may reach past N.  Stage by stage over the four: the same roundings as attn_score.
template <bool HAS_MASK>
__device__ __forceinline__ f32x4 attn_score4(f32x4 st, float ls, u32x4 bw, u32x4 mw, bool ragged, int kb, int N, float past) {
  const uint32_t b0 = bw.x, b1 = bw.y, b2 = bw.z, b3 = bw.w;
  float s0 = st[0] * ls + __uint_as_float(b0), s1 = st[1] * ls + __uint_as_float(b1);
  float s2 = st[2] * ls + __uint_as_float(b2), s3 = st[3] * ls + __uint_as_float(b3);
  if (HAS_MASK) {
    const uint32_t m0 = mw.x, m1 = mw.y, m2 = mw.z, m3 = mw.w;
    s0 += __uint_as_float(m0); s1 += __uint_as_float(m1); s2 += __uint_as_float(m2); s3 += __uint_as_float(m3);
  }
  if (ragged) {
    s0 = (kb + 0 < N) ? s0 : past; s1 = (kb + 1 < N) ? s1 : past;
    s2 = (kb + 2 < N) ? s2 : past; s3 = (kb + 3 < N) ? s3 : past;
  }
  st[0] = s0; st[1] = s1; st[2] = s2; st[3] = s3;
  return st;
}

// Online softmax, one block's step for one row: from the running maximum m_run, the ROUNDED reference point r_run = -m log2e the
// running sum's terms were made with, and the block's maximum bm, the new maximum (returned), the new reference point mneg and the
// factor alpha for the old sum and accumulators.  The old terms are 2^(x log2e + r_run): scaling by 2^(mneg - r_run) moves them to
// the new rounded reference point exactly, so the rounding of a reference point (up to 2^-17 in the exponent at logits near 100)
// cancels in the final division as it does in a one-pass softmax.  While the running maximum is still -inf (the first block) alpha
// is 0 without an exponential, on accumulators that are still 0; a block whose maximum is -inf (a caller's mask of -inf over a
// whole block) gets a zero reference point.
__device__ __forceinline__ float softmax_ref_step(float m_run, float r_run, float bm, float& mneg, float& alpha) {
  const float m_new = fmaxf(m_run, bm);
  mneg = (m_new == -INFINITY) ? 0.f : -m_new * L2E;
  alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mneg - r_run);
  return m_new;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// F.normalize backward for one (row, dim pair): y = x / max(n, eps); n >= eps: dx = (dy - y (y . dy)) / n, else dx = dy / eps
// (the clamp passes no gradient to the norm).  `dot` = y . dy over the row's 32 dims.
__device__ __forceinline__ float norm_bwd(float dy, float y, float dot, float n) {
  return n >= NEPS ? (dy - y * dot) / n : dy / NEPS;
}

// sum over the 16 lanes l15 of one lane group (xor butterfly: the same order on every call)
__device__ __forceinline__ float sum16(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// ---- host code only: the forward entry points' checks and launch preamble (host_launch.h style) ---------------------------------------
// The clauses every forward entry point has at the same place: unknown mode -> SDF_E_DTYPE; hd, B_, nH, n_lo <= N <= n_hi, a mask's
// nW, SEW's Tq * N1 == N -> SDF_E_SHAPE; else 0.
inline int sdf_win_attn_shape_rc(const SdfWinAttnDesc* d, int n_lo, int n_hi) {
  if (d->mode != SDF_ATTN_ANN && d->mode != SDF_ATTN_SEW) return SDF_E_DTYPE;
  if (d->hd != HD || d->B_ < 1 || d->nH < 1 || d->N < n_lo || d->N > n_hi) return SDF_E_SHAPE;
  if (d->mask && (d->nW < 1 || d->B_ % d->nW)) return SDF_E_SHAPE;
  if (d->mode == SDF_ATTN_SEW && (d->Tq < 1 || d->N1 < 1 || d->Tq * d->N1 != d->N)) return SDF_E_SHAPE;
  return 0;
}
// The desc a forward entry point accepts (sdf_win_attn_fwd, sdf_win_attn_large_fwd), as a value: SDF_E_NULL for a missing desc or
// pointer, the clauses above, SDF_E_NULL for a row map outside the ANN form or without the pad row, SDF_E_ALIGN; else 0.
// sdf_win_attn_scores_fwd orders its pointer, row-map and alignment clauses differently (no v, no out, k in SEW mode only) and keeps
// them; it shares sdf_win_attn_shape_rc, whose place among its checks is the same.
inline int sdf_win_attn_desc_rc(const SdfWinAttnDesc* d, int n_lo, int n_hi) {
  if (!d) return SDF_E_NULL;
  if (!d->q || !d->k || !d->v || !d->out || !d->scale || !d->bias) return SDF_E_NULL;
  if (const int rc = sdf_win_attn_shape_rc(d, n_lo, n_hi)) return rc;
  if (d->row_map && (d->mode != SDF_ATTN_ANN || !d->pad_qkv)) return SDF_E_NULL;   // windowing through the map: ANN form, needs the pad row
  if (!sdf_aligned(d->q, d->mode == SDF_ATTN_ANN ? 16 : 4) || !sdf_aligned(d->out, 4)) return SDF_E_ALIGN;
  return 0;
}
// the kernels' parameter block: the desc, with one mask window where there is no mask (b % nW stays defined)
inline AttnParams sdf_win_attn_params(const SdfWinAttnDesc* d) {
  AttnParams P;
  P.d = *d;
  if (!d->mask) P.d.nW = 1;
  return P;
}
// grid of the kernels whose workgroup is (window, head, 64 queries); 0 where it does not fit a grid dimension (SDF_E_SHAPE)
inline int64_t sdf_win_attn_group_grid(const SdfWinAttnDesc* d) {
  const int64_t groups = ((d->N + 15) / 16 + 3) / 4;
  const int64_t wgs = (int64_t)d->B_ * d->nH * groups;
  return wgs < (1LL << 31) ? wgs : 0;
}

}  // namespace
