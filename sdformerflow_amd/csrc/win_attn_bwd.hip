// Backward of the ANN cosine window attention (the core sdf_win_attn_fwd computes in SDF_ATTN_ANN mode), gfx950.
//
// Per window b and head g (reference models/STSwinNet/swin_transformer3D_v2.py:176-202):
//   q^ = q / max(|q|, 1e-12), k^ likewise;  S = q^ k^T * scale[g] + bias[g] (+ mask[b % nW]);  P = softmax(S);  O = P v
// Given dO:
//   dP = dO v^T,  D_i = rowsum(P o dP) (= rowsum(dO o O), formed from the recomputed P: the forward's output is not an input),
//   dS = P o (dP - D),  dv = P^T dO,  dq^ = scale dS k^,  dk^ = scale dS^T q^,
//   d_scale[g] = sum dS o (q^ k^T),  d_bias[g] = sum over windows of dS,  then the F.normalize backward on q^ and k^.
//
// One workgroup (4 waves) per (window, head); q^, k^, v and dO staged once in LDS (fp32), with the raw norms and, after the first
// pass, the row statistics (max, 1 / sum, D) of every query.
//   pass 1, query-major: a wave owns 16-query tiles and recomputes the 16 x N score strip in registers exactly as the forward's
//     general kernel does (S^T = K^ Q^^T on v_mfma_f32_16x16x4_f32: the accumulator of key tile jt is the A operand of the next
//     product), plus the dP strip (V dO^T, same layout); dS replaces P in place, goes to this window's d_bias slab, and
//     U = dS K^ gives dq^ = scale U and the d_scale term sum_i q^_i . U_i (= sum dS o q^k^T).
//   pass 2, key-major: a wave owns 16-key tiles and walks the query tiles: S and dP blocks with queries as rows, P from the
//     stored row statistics, dS; dv += P^T dO and dk^ += dS^T Q^ with the block as the A operand.
// Every product is the exact fp32 MFMA.  The cross-window sums (d_bias, d_scale, d_pad = the gradient of the padding tokens'
// q | k | v, i.e. of the qkv bias they read) are written per (window, head) to the workspace and summed in window order by a
// second kernel: no float atomics, two calls give bit-equal results.
// token_row, norm_bwd, sum16, load_row8 / mfma_row8, the score rounding and the workspace helpers are win_attn_common.h's.  Pass 1
// is not win_attn_large_bwd.hip's score_strip: folded on the tile count, this kernel went from 188 to 200 VGPRs.
#include "win_attn_common.h"

namespace {

constexpr int NT_MAX = 12;            // up to 192 tokens per window
constexpr int RED = 3 * HD + 1;       // per-wave partials: d_pad (q | k | v of one head) + d_scale

struct BwdParams {
  SdfWinAttnBwdDesc d;
  float* ws_bias;       // (B_, nH, NP, NP): dS of every (window, head)
  float* ws_scale;      // (B_, nH)
  float* ws_pad;        // (B_, nH, 96): dq | dk | dv of the window's padding tokens, this head's 32 dims each
};

__global__ __launch_bounds__(256) void win_attn_ann_bwd_kernel(BwdParams P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const SdfWinAttnBwdDesc& d = P.d;
  const int N = d.N, NT = (N + 15) / 16, NP = NT * 16;
  float* Qs = lds;                      // q^  [NP][LDW]
  float* Ks = Qs + NP * LDW;            // k^
  float* Vs = Ks + NP * LDW;            // v
  float* Gs = Vs + NP * LDW;            // dO (zero for padding tokens: their output is cropped)
  float* qn = Gs + NP * LDW;            // |q|, |k| per token
  float* kn = qn + NP;
  float* rm = kn + NP;                  // per query: row max, 1 / row sum, D
  float* rl = rm + NP;
  float* rD = rl + NP;
  float* red = rD + NP;                 // [4][RED]

  const int bg = blockIdx.x;
  const int b = bg / d.nH, g = bg - b * d.nH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lg = lane >> 4;
  const int C = d.nH * HD;
  const int64_t C3 = 3 * (int64_t)C;

  // ---- stage q^, k^, v, dO (one token row of 32 dims per thread) ----
  for (int r = tid; r < NP; r += 256) {
    float4 qv[8], kv[8], vv[8], gv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) qv[i] = kv[i] = vv[i] = gv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < N) {
      const int64_t row = token_row(d, b, r);
      const float* base = (row >= 0 ? d.qkv + row * C3 : d.pad_qkv) + g * HD;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        qv[i] = *reinterpret_cast<const float4*>(base + 4 * i);
        kv[i] = *reinterpret_cast<const float4*>(base + C + 4 * i);
        vv[i] = *reinterpret_cast<const float4*>(base + 2 * C + 4 * i);
      }
      if (row >= 0) {
        const float* gp = d.dout + row * C + g * HD;
#pragma unroll
        for (int i = 0; i < 8; ++i) gv[i] = *reinterpret_cast<const float4*>(gp + 4 * i);
      }
    }
    float sq = 0.f, sk = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sq += qv[i].x * qv[i].x + qv[i].y * qv[i].y + qv[i].z * qv[i].z + qv[i].w * qv[i].w;
      sk += kv[i].x * kv[i].x + kv[i].y * kv[i].y + kv[i].z * kv[i].z + kv[i].w * kv[i].w;
    }
    const float nq = sqrtf(sq), nk = sqrtf(sk);
    const float iq = 1.f / fmaxf(nq, NEPS), ik = 1.f / fmaxf(nk, NEPS);     // as the forward normalises
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      qv[i].x *= iq; qv[i].y *= iq; qv[i].z *= iq; qv[i].w *= iq;
      kv[i].x *= ik; kv[i].y *= ik; kv[i].z *= ik; kv[i].w *= ik;
      *reinterpret_cast<float4*>(&Qs[r * LDW + 4 * i]) = qv[i];
      *reinterpret_cast<float4*>(&Ks[r * LDW + 4 * i]) = kv[i];
      *reinterpret_cast<float4*>(&Vs[r * LDW + 4 * i]) = vv[i];
      *reinterpret_cast<float4*>(&Gs[r * LDW + 4 * i]) = gv[i];
    }
    qn[r] = nq;
    kn[r] = nk;
  }
  __syncthreads();

  const float ls = d.scale[g];
  const float* bias_g = d.bias + (int64_t)g * N * N;
  const float* mask_w = d.mask ? d.mask + (int64_t)(b % d.nW) * N * N : nullptr;
  float* slab = P.ws_bias + ((int64_t)b * d.nH + g) * NP * NP;
  // per-lane partials: d_pad of dims l15 / 16 + l15 for q, k, v (this lane's rows), d_scale
  float pq0 = 0.f, pq1 = 0.f, pk0 = 0.f, pk1 = 0.f, pv0 = 0.f, pv1 = 0.f, sacc = 0.f;

  // ================= pass 1: query tiles =================
  for (int qt = wave; qt < NT; qt += 4) {
    const int qi = qt * 16 + l15;                          // this lane's query (column of the S^T tiles)
    float qreg[8], greg[8];                                // q^[qi][8 lg + s], dO[qi][8 lg + s]
    load_row8(&Qs[qi * LDW + 8 * lg], qreg);
    load_row8(&Gs[qi * LDW + 8 * lg], greg);
    f32x4 st[NT_MAX], dp[NT_MAX];
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt) {
      if (jt < NT) {
        const int kj = jt * 16 + l15;                      // A operand row: key
        f32x4 acc = mfma_row8(&Ks[kj * LDW + 8 * lg], qreg);
        const f32x4 dacc = mfma_row8(&Vs[kj * LDW + 8 * lg], greg);
        // lane holds S[qi][kb + r], kb = 16 jt + 4 lg: scale, bias, mask (separately rounded, as the reference computes it)
        const int kb = jt * 16 + 4 * lg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool ok = qi < N && kb + r < N;
          const float bv = ok ? bias_g[(int64_t)qi * N + kb + r] : 0.f;
          const float mv = (ok && mask_w) ? mask_w[(int64_t)qi * N + kb + r] : 0.f;
          acc[r] = attn_score(acc[r], ls, bv, mv, kb + r < N, -INFINITY);
        }
        st[jt] = acc;
        dp[jt] = dacc;
      }
    }
    // softmax row statistics (the four lane groups hold the same query)
    float m = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt)
      if (jt < NT) m = fmaxf(fmaxf(fmaxf(m, st[jt][0]), fmaxf(st[jt][1], st[jt][2])), st[jt][3]);
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt)
      if (jt < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = expf(st[jt][r] - m);
          st[jt][r] = e;
          sum += e;
        }
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
    // D = rowsum(P o dP) = dO . O, with the P recomputed here (exact fp32, consistent with the dS below)
    float Dq = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt)
      if (jt < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[jt][r] *= inv;
          Dq += st[jt][r] * dp[jt][r];
        }
      }
    Dq += __shfl_xor(Dq, 16);
    Dq += __shfl_xor(Dq, 32);
    if (lg == 0) {
      rm[qi] = m;
      rl[qi] = inv;
      rD[qi] = Dq;
    }
    // dS = P o (dP - D), in place of P; this window's d_bias slab (NP x NP, 16-byte aligned rows)
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt)
      if (jt < NT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) st[jt][r] = st[jt][r] * (dp[jt][r] - Dq);
        if (qi < N) *reinterpret_cast<f32x4*>(&slab[(int64_t)qi * NP + jt * 16 + 4 * lg]) = st[jt];
      }
    // U = dS K^ : A = dS (registers), B = K^[key = 16 jt + 4 lg + s][dim = 16 dt + l15]
    f32x4 u0 = {0.f, 0.f, 0.f, 0.f}, u1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < NT_MAX; ++jt)
      if (jt < NT) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int key = jt * 16 + 4 * lg + s;
          u0 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][s], Ks[key * LDW + l15], u0, 0, 0, 0);
          u1 = __builtin_amdgcn_mfma_f32_16x16x4f32(st[jt][s], Ks[key * LDW + 16 + l15], u1, 0, 0, 0);
        }
      }
    // u[r] = U[query qt*16 + 4 lg + r][dim l15 | 16 + l15]: d_scale term, dq^ = scale U, normalize backward, store
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = qt * 16 + 4 * lg + r;
      const float y0 = Qs[i * LDW + l15], y1 = Qs[i * LDW + 16 + l15];
      sacc += y0 * u0[r] + y1 * u1[r];
      const float dy0 = ls * u0[r], dy1 = ls * u1[r];
      const float dot = sum16(y0 * dy0 + y1 * dy1);
      const float n = qn[i];
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
  __syncthreads();

  // ================= pass 2: key tiles =================
  for (int kt = wave; kt < NT; kt += 4) {
    const int kj = kt * 16 + l15;                          // this lane's key (column of the S / dP blocks)
    float kreg[8], vreg[8];                                // k^[kj][8 lg + s], v[kj][8 lg + s]
    load_row8(&Ks[kj * LDW + 8 * lg], kreg);
    load_row8(&Vs[kj * LDW + 8 * lg], vreg);
    f32x4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = {0.f, 0.f, 0.f, 0.f}, dk0 = {0.f, 0.f, 0.f, 0.f}, dk1 = {0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < NT; ++it) {
      const int qa = it * 16 + l15;                        // A operand row: query
      const f32x4 acc = mfma_row8(&Qs[qa * LDW + 8 * lg], kreg);
      const f32x4 dacc = mfma_row8(&Gs[qa * LDW + 8 * lg], vreg);
      // lane holds S / dP [query it*16 + 4 lg + r][key kj]: P from the stored row statistics, dS
      float p[4], ds[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = it * 16 + 4 * lg + r;
        const bool ok = i < N && kj < N;
        const float bv = ok ? bias_g[(int64_t)i * N + kj] : 0.f;
        const float mv = (ok && mask_w) ? mask_w[(int64_t)i * N + kj] : 0.f;
        const float sc = attn_score(acc[r], ls, bv, mv, true, 0.f);
        p[r] = ok ? expf(sc - rm[i]) * rl[i] : 0.f;
        ds[r] = p[r] * (dacc[r] - rD[i]);
      }
      // dv += P^T dO, dk^/scale += dS^T Q^ : A = the block (row key l15, k = query 4 lg + s), B = dO / q^[query][dim 16 dt + l15]
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int q = it * 16 + 4 * lg + s;
        dv0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], Gs[q * LDW + l15], dv0, 0, 0, 0);
        dv1 = __builtin_amdgcn_mfma_f32_16x16x4f32(p[s], Gs[q * LDW + 16 + l15], dv1, 0, 0, 0);
        dk0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[s], Qs[q * LDW + l15], dk0, 0, 0, 0);
        dk1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[s], Qs[q * LDW + 16 + l15], dk1, 0, 0, 0);
      }
    }
    // dv0[r] = dv[key kt*16 + 4 lg + r][dim l15]; dk^ = scale dk; normalize backward; store
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = kt * 16 + 4 * lg + r;
      const float y0 = Ks[j * LDW + l15], y1 = Ks[j * LDW + 16 + l15];
      const float dy0 = ls * dk0[r], dy1 = ls * dk1[r];
      const float dot = sum16(y0 * dy0 + y1 * dy1);
      const float n = kn[j];
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

  // ---- per-(window, head) partials: lane groups, then waves in a fixed order ----
  float part[6] = {pq0, pq1, pk0, pk1, pv0, pv1};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    part[i] += __shfl_xor(part[i], 16);
    part[i] += __shfl_xor(part[i], 32);
  }
  sacc = sum16(sacc);
  sacc += __shfl_xor(sacc, 16);
  sacc += __shfl_xor(sacc, 32);
  if (lg == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) red[wave * RED + 16 * i + l15] = part[i];
  }
  if (lane == 0) red[wave * RED + 3 * HD] = sacc;
  __syncthreads();
  if (tid < RED) {
    const float v = ((red[tid] + red[RED + tid]) + red[2 * RED + tid]) + red[3 * RED + tid];
    if (tid < 3 * HD) P.ws_pad[(int64_t)bg * 3 * HD + tid] = v;
    else P.ws_scale[bg] = v;
  }
}

// Cross-window sums in window order: d_bias (nH, N, N), d_scale (nH), d_pad (3C).  One thread per output element.
__global__ __launch_bounds__(256) void win_attn_ann_bwd_reduce_kernel(BwdParams P) {
  const SdfWinAttnBwdDesc& d = P.d;
  const int N = d.N, NP = padded_n(N), B_ = d.B_, nH = d.nH, C = nH * HD;
  const int64_t nb = (int64_t)nH * N * N;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < nb) {
    const int g = (int)(idx / ((int64_t)N * N));
    const int rem = (int)(idx - (int64_t)g * N * N);
    const int i = rem / N, j = rem - i * N;
    const float* p = P.ws_bias + ((int64_t)g * NP + i) * NP + j;
    const int64_t stride = (int64_t)nH * NP * NP;
    float s = 0.f;
    int w = 0;
    for (; w + 8 <= B_; w += 8) {                          // eight loads in flight, added in window order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(w + u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; w < B_; ++w) s += p[(int64_t)w * stride];
    d.d_bias[idx] = s;
  } else if (idx < nb + nH) {
    const int g = (int)(idx - nb);
    float s = 0.f;
    for (int w = 0; w < B_; ++w) s += P.ws_scale[(int64_t)w * nH + g];
    d.d_scale[g] = s;
  } else if (idx < nb + nH + 3 * C) {
    const int c = (int)(idx - nb - nH);
    const int part = c / C, rest = c - part * C, g = rest / HD, dd = rest - g * HD;
    float s = 0.f;
    for (int w = 0; w < B_; ++w) s += P.ws_pad[((int64_t)w * nH + g) * 3 * HD + part * HD + dd];
    if (d.d_pad) d.d_pad[c] = s;
  }
}

size_t bwd_lds_bytes(int N) {
  const int NP = padded_n(N);
  return (size_t)(4 * NP * LDW + 5 * NP + 4 * RED) * sizeof(float);
}

}  // namespace

extern "C" int64_t sdf_win_attn_ann_bwd_workspace_bytes(int B_, int nH, int N) {
  if (B_ < 1 || nH < 1 || N < 1 || N > 16 * NT_MAX) return 0;
  const int64_t NP = padded_n(N), bh = (int64_t)B_ * nH;
  return align256(bh * NP * NP * 4) + align256(bh * 4) + align256(bh * 3 * HD * 4);
}

extern "C" int sdf_win_attn_ann_bwd(const SdfWinAttnBwdDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (!d->qkv || !d->dout || !d->scale || !d->bias || !d->dqkv || !d->d_scale || !d->d_bias || !d->workspace)
    return SDF_E_NULL;
  if (d->row_map && (!d->pad_qkv || !d->d_pad)) return SDF_E_NULL;       // windowing through the map: needs the pad row and its gradient
  if (d->hd != HD || d->B_ < 1 || d->nH < 1 || d->N < 1 || d->N > 16 * NT_MAX) return SDF_E_SHAPE;
  if (d->mask && (d->nW < 1 || d->B_ % d->nW)) return SDF_E_SHAPE;
  if (d->workspace_bytes < sdf_win_attn_ann_bwd_workspace_bytes(d->B_, d->nH, d->N)) return SDF_E_SHAPE;
  if (!sdf_aligned(d->qkv, 16) || !sdf_aligned(d->dout, 16) || !sdf_aligned(d->dqkv, 4) ||
      !sdf_aligned(d->workspace, 256) || (d->pad_qkv && !sdf_aligned(d->pad_qkv, 16)))
    return SDF_E_ALIGN;
  BwdParams P;
  P.d = *d;
  if (!d->mask) P.d.nW = 1;
  const int64_t NP = padded_n(d->N), bh = (int64_t)d->B_ * d->nH;
  char* ws = reinterpret_cast<char*>(d->workspace);
  P.ws_bias = reinterpret_cast<float*>(ws);
  P.ws_scale = reinterpret_cast<float*>(ws + align256(bh * NP * NP * 4));
  P.ws_pad = reinterpret_cast<float*>(ws + align256(bh * NP * NP * 4) + align256(bh * 4));
  static std::atomic<uint64_t> opt{0};                       // > 64 KiB of dynamic LDS: opt-in once per device
  if (const int e = sdf_lds_opt_in(opt, reinterpret_cast<const void*>(win_attn_ann_bwd_kernel), (int)bwd_lds_bytes(16 * NT_MAX))) return e;
  hipStream_t s = sdf_stream(stream);
  SDF_LAUNCH(win_attn_ann_bwd_kernel, dim3((unsigned)bh), dim3(256), bwd_lds_bytes(d->N), s, P);
  SDF_LAUNCH_CHECK();
  const int64_t total = (int64_t)d->nH * d->N * d->N + d->nH + 3 * (int64_t)d->nH * HD;
  SDF_LAUNCH(win_attn_ann_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, P);
  SDF_LAUNCH_CHECK();
  return 0;
}
