// Signed voxel volume -> the model's input, gfx950: harness.prepare_chunk(center_crop(voxel, crop), norm_input, spike_th, polarity=True)
// (reference eval_DSEC_flow_SNN.py:179-217) without a host round trip.
//
// The torch composition asks the host three times (nz.any(), chunk[nz], lo != hi); here the decisions stay on the device.  Every
// operation is IEEE fp32 in both, so the output equals the composition bit for bit.  min / max of the non-zeros are integer atomics on
// bit patterns (the values are positive floats, which order as their bit patterns: any arrival order gives the same pair), one pair per
// workgroup; the minimum is kept as the maximum of the complemented pattern, so that "no non-zero element" is all-zero for both words.
//
// Launch sequence: [clear the pairs] | split (+ min / max) | [finish: min-max, threshold, event mask].
//
// sdf_augment_chunk_fwd is the training loops' front of the same preparation (reference train_flow_parallel_supervised_SNN.py:155-171,
// :241-308; DSEC_dataloader/data_augmentation.py): its first kernel gathers a per-sample crop window with flips and the event drop - of
// the voxel, the flow and the valid mask - before the split; the finish kernel is shared.
#include "common.h"

namespace {

struct PcGeom {
  int32_t B, bins, Hs, Ws, oy, ox, h, w;
};

// relu as ATen's device clamp_min forms it: NaN stays, else fmaxf(v, 0) = v_max_f32, which orders -0 below +0: relu(-0) = +0
__device__ __forceinline__ float pc_relu(float v) { return v != v ? v : fmaxf(v, 0.f); }

// sample blockIdx.y, cells strided over the sample's gridDim.x workgroups: out = relu(v) | relu(-v) on the crop window, and the pair
// {~min, max} of the bit patterns of the non-zeros into mm[2 g], g = the sample (per_sample) or 0 (the whole batch tensor)
__global__ __launch_bounds__(256) void prepare_split_kernel(const float* __restrict__ voxel, float* __restrict__ out, PcGeom g,
                                                            unsigned* __restrict__ mm, int want_minmax, int per_sample) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int hw = g.h * g.w;
  const int cells = g.bins * hw;                                           // (< 2^31: pc_geom)
  const float* src = voxel + (int64_t)b * g.bins * g.Hs * g.Ws;
  float* dst = out + (int64_t)b * 2 * cells;
  unsigned nlo = 0u, hi = 0u;                                              // (~min, max) over nothing
  for (int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x; i64 < cells; i64 += (int64_t)gridDim.x * 256) {
    const int i = (int)i64, c = i / hw, p = i - c * hw;
    const int y = p / g.w, x = p % g.w;
    const float v = src[((int64_t)c * g.Hs + g.oy + y) * g.Ws + g.ox + x];
    const float o1 = pc_relu(v), o2 = pc_relu(-v);
    dst[(int64_t)c * 2 * hw + p] = o1;
    dst[(int64_t)c * 2 * hw + hw + p] = o2;
    if (o1 != 0.f) {
      nlo = max(nlo, ~__float_as_uint(o1));
      hi = max(hi, __float_as_uint(o1));
    }
    if (o2 != 0.f) {
      nlo = max(nlo, ~__float_as_uint(o2));
      hi = max(hi, __float_as_uint(o2));
    }
  }
  if (!want_minmax) return;
  for (int off = 32; off > 0; off >>= 1) {
    nlo = max(nlo, (unsigned)__shfl_xor((int)nlo, off));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
  }
  // one pair of atomics per workgroup: same-address atomics serialise in L2, and a pair per wave cost more than the pass itself
  __shared__ unsigned red[4][2];
  if (lane == 0) {
    red[threadIdx.x >> 6][0] = nlo;
    red[threadIdx.x >> 6][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nlo = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
    hi = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    if (hi != 0u) {
      unsigned* q = mm + 2 * (per_sample ? b : 0);
      atomicMax(&q[0], nlo);
      atomicMax(&q[1], hi);
    }
  }
}

// the per-sample parameters of sdf_augment_chunk_fwd, copied from the descriptor's host arrays into the kernel arguments (832 bytes)
struct AugParams {
  int32_t oy[SDF_AUGMENT_MAX_B], ox[SDF_AUGMENT_MAX_B];
  float q[SDF_AUGMENT_MAX_B];
  uint8_t flags[SDF_AUGMENT_MAX_B];
};

// Philox4x32-10 (Salmon et al., SC'11): word `i & 3` of the block at counter (i >> 2, offset) under key `seed`, as u = (word >> 8) 2^-24
__device__ __forceinline__ float aug_philox_u(uint64_t i, uint64_t seed, uint64_t offset) {
  uint32_t c0 = (uint32_t)(i >> 2), c1 = (uint32_t)(i >> 34), c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const int j = (int)(i & 3);
  const uint32_t word = j == 0 ? c0 : j == 1 ? c1 : j == 2 ? c2 : c3;
  return (float)(word >> 8) * 0x1p-24f;
}

// The training loops' Compose([RandomCrop, flips, Random_event_drop]) and the polarity split in one pass, laid out as prepare_split_kernel
// (sample blockIdx.y, cells strided over the sample's workgroups): output cell (c, y, x) reads the source at
// (oy + (vflip ? h-1-y : y), ox + (hflip ? w-1-x : x)) - the stores run forwards and stay coalesced, a flipped row is loaded backwards -
// then v *= (u > q) for a sample that drops (u from `drop_u` in output coordinates, else Philox at the cell's index in (B, bins, h, w)),
// then relu(v) | relu(-v) and the {~min, max} pair.  Behind the cells the same workgroups gather the flow (x negated under hflip, y under
// vflip) and the valid mask (as 0.f / 1.f).
__global__ __launch_bounds__(256) void augment_split_kernel(const float* __restrict__ voxel, const float* __restrict__ label,
                                                            const void* __restrict__ valid, const float* __restrict__ drop_u,
                                                            float* __restrict__ out, float* __restrict__ label_out,
                                                            float* __restrict__ mask_out, PcGeom g, AugParams a, unsigned* __restrict__ mm,
                                                            int want_minmax, int per_sample, int valid_is_u8, uint64_t seed, uint64_t offset) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int hw = g.h * g.w;
  const int cells = g.bins * hw;                                           // (< 2^30: aug_geom)
  const int oy = a.oy[b], ox = a.ox[b];
  const bool hflip = a.flags[b] & 1, vflip = a.flags[b] & 2;
  const float q = a.q[b];
  const bool drop = !(q < 0.f);
  const int64_t plane = (int64_t)g.Hs * g.Ws;
  const float* src = voxel + (int64_t)b * g.bins * plane;
  float* dst = out + (int64_t)b * 2 * cells;
  unsigned nlo = 0u, hi = 0u;                                              // (~min, max) over nothing
  for (int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x; i64 < cells; i64 += (int64_t)gridDim.x * 256) {
    const int i = (int)i64, c = i / hw, p = i - c * hw;
    const int y = p / g.w, x = p % g.w;
    const int sy = oy + (vflip ? g.h - 1 - y : y), sx = ox + (hflip ? g.w - 1 - x : x);
    float v = src[c * plane + (int64_t)sy * g.Ws + sx];
    if (drop) {
      const int64_t cell = (int64_t)b * cells + i;
      const float u = drop_u ? drop_u[cell] : aug_philox_u((uint64_t)cell, seed, offset);
      v = v * (u > q ? 1.f : 0.f);
    }
    const float o1 = pc_relu(v), o2 = pc_relu(-v);
    dst[(int64_t)c * 2 * hw + p] = o1;
    dst[(int64_t)c * 2 * hw + hw + p] = o2;
    if (o1 != 0.f) {
      nlo = max(nlo, ~__float_as_uint(o1));
      hi = max(hi, __float_as_uint(o1));
    }
    if (o2 != 0.f) {
      nlo = max(nlo, ~__float_as_uint(o2));
      hi = max(hi, __float_as_uint(o2));
    }
  }
  if (label || valid) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
      const int y = p / g.w, x = p % g.w;
      const int64_t s = (int64_t)(oy + (vflip ? g.h - 1 - y : y)) * g.Ws + ox + (hflip ? g.w - 1 - x : x);
      if (label) {
        const float fx = label[(int64_t)b * 2 * plane + s], fy = label[((int64_t)b * 2 + 1) * plane + s];
        label_out[(int64_t)b * 2 * hw + p] = hflip ? -fx : fx;
        label_out[(int64_t)b * 2 * hw + hw + p] = vflip ? -fy : fy;
      }
      if (valid) {
        const bool on = valid_is_u8 ? static_cast<const uint8_t*>(valid)[b * plane + s] != 0
                                    : static_cast<const float*>(valid)[b * plane + s] != 0.f;
        mask_out[(int64_t)b * hw + p] = on ? 1.f : 0.f;
      }
    }
  }
  if (!want_minmax) return;
  for (int off = 32; off > 0; off >>= 1) {
    nlo = max(nlo, (unsigned)__shfl_xor((int)nlo, off));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
  }
  __shared__ unsigned red[4][2];                                           // one pair of atomics per workgroup, as prepare_split_kernel
  if (lane == 0) {
    red[threadIdx.x >> 6][0] = nlo;
    red[threadIdx.x >> 6][1] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nlo = max(max(red[0][0], red[1][0]), max(red[2][0], red[3][0]));
    hi = max(max(red[0][1], red[1][1]), max(red[2][1], red[3][1]));
    if (hi != 0u) {
      unsigned* r = mm + 2 * (per_sample ? b : 0);
      atomicMax(&r[0], nlo);
      atomicMax(&r[1], hi);
    }
  }
}

// prepare_chunk's tail, one lane per pixel of a sample over its 2 bins planes: (v - lo) / (hi - lo) on the non-zeros when there are any
// and lo != hi; the spike threshold (> th: 1, < th: 0, == th: kept); and the event mask, chunk.sum(1).sum(1).bool(): the values are
// non-negative here, so their sum is non-zero exactly when one of them is.  `mul` (the training loop's mask * event_mask; may be NULL):
// (B, 1, h, w) fp32, multiplied by the event mask in place
__global__ __launch_bounds__(256) void prepare_finish_kernel(float* __restrict__ out, float* __restrict__ mask, int64_t pixels, int hw,
                                                             int planes, const unsigned* __restrict__ mm, int want_minmax, int per_sample,
                                                             int want_th, float th, float* __restrict__ mul) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  const int64_t b = i / hw;
  bool norm = false;
  float lo = 0.f, span = 1.f;
  if (want_minmax) {
    const unsigned* q = mm + 2 * (per_sample ? b : 0);
    const unsigned lob = ~q[0], hib = q[1];
    lo = __uint_as_float(lob);
    span = __uint_as_float(hib) - lo;
    norm = hib != 0u && lob != hib;
  }
  float* q = out + b * planes * hw + i % hw;
  bool any = false;
  const bool write = norm || want_th;
  for (int j = 0; j < planes; ++j) {
    float v = q[(int64_t)j * hw];
    if (norm && v != 0.f) v = (v - lo) / span;
    if (want_th) v = v > th ? 1.f : (v < th ? 0.f : v);
    if (write) q[(int64_t)j * hw] = v;
    any = any || v != 0.f;
  }
  if (mask) mask[i] = any ? 1.f : 0.f;
  if (mul) mul[i] = mul[i] * (any ? 1.f : 0.f);
}

// geometry check; false = SDF_E_SHAPE
bool pc_geom(const SdfPrepareChunkDesc* d, PcGeom& g) {
  if (d->B < 1 || d->B > 65535 || d->bins < 1 || d->Hs < 1 || d->Ws < 1 || d->crop_h < 0 || d->crop_w < 0) return false;
  if ((d->crop_h == 0) != (d->crop_w == 0) || d->crop_oy < 0 || d->crop_ox < 0) return false;
  if (d->crop_h == 0 && (d->crop_oy || d->crop_ox)) return false;
  if ((int64_t)d->crop_oy + d->crop_h > d->Hs || (int64_t)d->crop_ox + d->crop_w > d->Ws) return false;      // the window lies inside the volume
  g.B = d->B;
  g.bins = d->bins;
  g.Hs = d->Hs;
  g.Ws = d->Ws;
  g.oy = d->crop_oy;
  g.ox = d->crop_ox;
  g.h = d->crop_h ? d->crop_h : d->Hs;
  g.w = d->crop_w ? d->crop_w : d->Ws;
  if ((int64_t)g.bins * g.h * g.w >= (1ll << 30) || (int64_t)g.B * g.bins * 2 * g.h * g.w >= (1ll << 40)) return false;
  return (int64_t)g.B * g.bins * g.Hs * g.Ws < (1ll << 40);
}

// geometry check of sdf_augment_chunk_fwd, every sample's origin included, and the kernel's copy of the per-sample arrays; false =
// SDF_E_SHAPE.  The kernel reads rows oy .. oy + h - 1 and columns ox .. ox + w - 1 of a sample, whatever its flips.
bool aug_geom(const SdfAugmentChunkDesc* d, PcGeom& g, AugParams& a) {
  if (d->B < 1 || d->B > SDF_AUGMENT_MAX_B || d->bins < 1 || d->Hs < 1 || d->Ws < 1 || d->crop_h < 0 || d->crop_w < 0) return false;
  if ((d->crop_h == 0) != (d->crop_w == 0) || d->crop_h > d->Hs || d->crop_w > d->Ws) return false;
  g.B = d->B;
  g.bins = d->bins;
  g.Hs = d->Hs;
  g.Ws = d->Ws;
  g.oy = g.ox = 0;                                                         // (per sample: AugParams)
  g.h = d->crop_h ? d->crop_h : d->Hs;
  g.w = d->crop_w ? d->crop_w : d->Ws;
  if ((int64_t)g.bins * g.h * g.w >= (1ll << 30) || (int64_t)g.bins * g.Hs * g.Ws >= (1ll << 34)) return false;
  for (int b = 0; b < SDF_AUGMENT_MAX_B; ++b) {
    const bool used = b < g.B;
    if (used && (d->oy[b] < 0 || d->ox[b] < 0 || d->oy[b] > g.Hs - g.h || d->ox[b] > g.Ws - g.w)) return false;
    a.oy[b] = used ? d->oy[b] : 0;
    a.ox[b] = used ? d->ox[b] : 0;
    a.q[b] = used ? d->drop_q[b] : -1.f;
    a.flags[b] = used ? (uint8_t)(d->flags[b] & 3) : 0;
  }
  return true;
}

}  // namespace

extern "C" int64_t sdf_prepare_chunk_workspace_bytes(int B) { return B >= 1 && B <= 65535 ? (int64_t)8 * B : 0; }

extern "C" int sdf_prepare_chunk_fwd(const SdfPrepareChunkDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  PcGeom g;
  if (!pc_geom(d, g)) return SDF_E_SHAPE;
  if (d->norm < 0 || d->norm > 1) return SDF_E_DTYPE;                      // 0 none | 1 min-max ("std" stays the torch function's)
  if (!d->voxel || !d->out || !d->workspace) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)8 * d->B) return SDF_E_SHAPE;
  if (!sdf_aligned(d->voxel, 4) || !sdf_aligned(d->out, 4) || !sdf_aligned(d->event_mask, 4) || !sdf_aligned(d->workspace, 8))
    return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  unsigned* mm = static_cast<unsigned*>(d->workspace);
  const int per_sample = d->per_sample != 0, want_minmax = d->norm == 1;
  if (want_minmax) {
    const hipError_t e = hipMemsetAsync(mm, 0, (size_t)8 * (per_sample ? g.B : 1), s);     // every pair: no non-zero element
    if (e != hipSuccess) return (int)e;
  }
  const int hw = g.h * g.w;
  const int64_t cells = (int64_t)g.bins * hw;
  // at most 1024 workgroups in all (one atomic pair each), at least one per sample
  const int64_t cap = 1024 / g.B > 1 ? 1024 / g.B : 1, need = (cells + 255) / 256;
  const dim3 block(256), sgrid((unsigned)(need < cap ? need : cap), g.B);
  SDF_LAUNCH(prepare_split_kernel, sgrid, block, 0, s, d->voxel, d->out, g, mm, want_minmax, per_sample);
  SDF_LAUNCH_CHECK();
  if (want_minmax || d->use_spike_th || d->event_mask) {
    const int64_t pixels = (int64_t)g.B * hw;
    SDF_LAUNCH(prepare_finish_kernel, dim3((unsigned)((pixels + 255) / 256)), block, 0, s, d->out, d->event_mask, pixels, hw, 2 * g.bins, mm,
               want_minmax, per_sample, d->use_spike_th, d->spike_th, (float*)nullptr);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int64_t sdf_augment_chunk_workspace_bytes(int B) { return B >= 1 && B <= SDF_AUGMENT_MAX_B ? (int64_t)8 * B : 0; }

extern "C" int sdf_augment_chunk_fwd(const SdfAugmentChunkDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  PcGeom g;
  AugParams a;
  if (!aug_geom(d, g, a)) return SDF_E_SHAPE;                              // every sample's window lies inside the volume
  if (d->norm < 0 || d->norm > 1) return SDF_E_DTYPE;                      // 0 none | 1 min-max ("std" stays the torch function's)
  for (int b = 0; b < g.B; ++b)
    if (d->flags[b] & ~3) return SDF_E_DTYPE;                              // bit 0 horizontal, bit 1 vertical
  if (!d->voxel || !d->out || !d->workspace) return SDF_E_NULL;
  if (!d->label != !d->label_out || !d->valid != !d->mask_out) return SDF_E_NULL;          // an input and its output come together
  if (d->mask_events && !d->mask_out) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)8 * d->B) return SDF_E_SHAPE;
  if (!sdf_aligned(d->voxel, 4) || !sdf_aligned(d->label, 4) || !sdf_aligned(d->drop_u, 4) || !sdf_aligned(d->out, 4) ||
      !sdf_aligned(d->label_out, 4) || !sdf_aligned(d->mask_out, 4) || !sdf_aligned(d->event_mask, 4) || !sdf_aligned(d->workspace, 8) ||
      (!d->valid_is_u8 && !sdf_aligned(d->valid, 4)))
    return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  unsigned* mm = static_cast<unsigned*>(d->workspace);
  const int per_sample = d->per_sample != 0, want_minmax = d->norm == 1;
  if (want_minmax) {
    const hipError_t e = hipMemsetAsync(mm, 0, (size_t)8 * (per_sample ? g.B : 1), s);     // every pair: no non-zero element
    if (e != hipSuccess) return (int)e;
  }
  const int hw = g.h * g.w;
  const int64_t cells = (int64_t)g.bins * hw;
  // the grid of sdf_prepare_chunk_fwd: at most 1024 workgroups in all (one atomic pair each), at least one per sample
  const int64_t cap = 1024 / g.B > 1 ? 1024 / g.B : 1, need = (cells + 255) / 256;
  const dim3 block(256), sgrid((unsigned)(need < cap ? need : cap), g.B);
  SDF_LAUNCH(augment_split_kernel, sgrid, block, 0, s, d->voxel, d->label, d->valid, d->drop_u, d->out, d->label_out, d->mask_out, g, a, mm,
             want_minmax, per_sample, d->valid_is_u8 != 0, (uint64_t)d->seed, (uint64_t)d->offset);
  SDF_LAUNCH_CHECK();
  float* mul = d->mask_events ? d->mask_out : nullptr;
  if (want_minmax || d->use_spike_th || d->event_mask || mul) {
    const int64_t pixels = (int64_t)g.B * hw;
    SDF_LAUNCH(prepare_finish_kernel, dim3((unsigned)((pixels + 255) / 256)), block, 0, s, d->out, d->event_mask, pixels, hw, 2 * g.bins, mm,
               want_minmax, per_sample, d->use_spike_th, d->spike_th, mul);
    SDF_LAUNCH_CHECK();
  }
  return 0;
}
