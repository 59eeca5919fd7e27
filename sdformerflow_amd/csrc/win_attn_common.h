// What the window-attention forward files (win_attn.hip, win_attn_large.hip) share: the head dimension, the padded LDS row, the kernel
// parameter block and the ANN mode's row lookup.  win_attn_large_bwd.hip takes the head dimension and the padded row from here.
#pragma once
#include "device_prims.h"

namespace {

constexpr int HD = 32;
constexpr int LDW = HD + 4;           // padded LDS row (floats)

struct AttnParams {
  SdfWinAttnDesc d;
};

// ANN mode: first float of the q | k | v row of token r of window b.  With a row map the window partition (pad, roll, reshape)
// is this lookup; a padding token reads the qkv Linear's image of a zero row.
__device__ __forceinline__ const float* qkv_row(const SdfWinAttnDesc& d, int b, int r, int C) {
  const float* q = reinterpret_cast<const float*>(d.q);
  if (!d.row_map) return q + ((int64_t)b * d.N + r) * 3 * C;
  const int row = d.row_map[(int64_t)b * d.N + r];
  return row >= 0 ? q + (int64_t)row * 3 * C : d.pad_qkv;
}

}  // namespace
