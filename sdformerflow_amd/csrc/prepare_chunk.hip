// Signed voxel volume -> the model's input, gfx950: harness.prepare_chunk(center_crop(voxel, crop), norm_input, spike_th, polarity=True)
// (reference eval_DSEC_flow_SNN.py:179-217) without a host round trip.
//
// The torch composition asks the host three times (nz.any(), chunk[nz], lo != hi); here the decisions stay on the device.  Every
// operation is IEEE fp32 in both, so the output equals the composition bit for bit.  The split's store, the min / max pairs (one pair of
// integer atomics per workgroup), their clear and the finish kernel are model_input.h's, shared with the voxel front ends.
//
// Launch sequence: [clear the pairs] | split (+ min / max) | [finish: min-max, threshold, event mask].
//
// sdf_augment_chunk_fwd is the training loops' front of the same preparation (reference train_flow_parallel_supervised_SNN.py:155-171,
// :241-308; DSEC_dataloader/data_augmentation.py): its first kernel gathers a per-sample crop window with flips and the event drop - of
// the voxel, the flow and the valid mask - before the split; the finish kernel is shared.
//
// sdf_augment_resize_fwd is the MDR training items' front (reference MDR_dataloader/loader_utils.py DenseSparseAugmentor, MDR.py:218-241,
// train_mdr_supervised_SNN.py:209-276): its first kernel gathers through a per-sample bilinear rescale (cv2.resize INTER_LINEAR restated,
// four taps), the flips and the crop - of the old and new dense event volumes and of the flow, which it scales and from which it derives
// the valid mask - before the same split; the finish kernel is shared.
#include "model_input.h"
#include <cmath>

namespace {

struct PcGeom {
  int32_t B, bins, Hs, Ws, oy, ox, h, w;
};

// sample blockIdx.y, cells strided over the sample's gridDim.x workgroups: out = relu(v) | relu(-v) on the crop window, and the pair
// {~min, max} of the bit patterns of the non-zeros into mm[2 g], g = the sample (per_sample) or 0 (the whole batch tensor)
__global__ __launch_bounds__(256) void prepare_split_kernel(const float* __restrict__ voxel, float* __restrict__ out, PcGeom g,
                                                            unsigned* __restrict__ mm, int want_minmax, int per_sample) {
  const int b = blockIdx.y;
  const int hw = g.h * g.w;
  const int cells = g.bins * hw;                                           // (< 2^31: pc_geom)
  const float* src = voxel + (int64_t)b * g.bins * g.Hs * g.Ws;
  float* dst = out + (int64_t)b * 2 * cells;
  unsigned nlo = 0u, hi = 0u;                                              // (~min, max) over nothing
  for (int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x; i64 < cells; i64 += (int64_t)gridDim.x * 256) {
    const int i = (int)i64, c = i / hw, p = i - c * hw;
    const int y = p / g.w, x = p % g.w;
    const float v = src[((int64_t)c * g.Hs + g.oy + y) * g.Ws + g.ox + x];
    mi_split_store(v, dst + (int64_t)c * 2 * hw + p, hw, nlo, hi);
  }
  if (want_minmax) mi_minmax_commit(nlo, hi, mm + 2 * (per_sample ? b : 0));
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
  const int b = blockIdx.y;
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
    mi_split_store(v, dst + (int64_t)c * 2 * hw + p, hw, nlo, hi);
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
  if (want_minmax) mi_minmax_commit(nlo, hi, mm + 2 * (per_sample ? b : 0));
}

// the per-sample parameters of sdf_augment_resize_fwd in the kernel arguments (2624 bytes): the position in the resized image of output
// pixel (y, x) is (by + sy y, bx + sx x), sy / sx = -1 under a flip (flags bit 1 / bit 0), by / bx = the origin in the flipped image
// taken back through the flips; inv = 1 / scale and mul = the flow's factor, scale * sign (1 or -1 for a sample that is not resized:
// flags bit 2 clear)
struct RzParams {
  double inv_x[SDF_AUGMENT_MAX_B], inv_y[SDF_AUGMENT_MAX_B], mul_x[SDF_AUGMENT_MAX_B], mul_y[SDF_AUGMENT_MAX_B];
  int32_t by[SDF_AUGMENT_MAX_B], bx[SDF_AUGMENT_MAX_B];
  uint8_t flags[SDF_AUGMENT_MAX_B];
};

// one axis of cv2.resize(INTER_LINEAR) as OpenCV forms it: destination index d of a source of n elements at inverse scale `inv` ->
// taps i0, i1 = min(i0 + 1, n - 1) and the weight a of the second; c = (float)((d + 0.5) inv - 0.5) with the product and the difference
// in double, i0 = floor(c), a = c - i0 in float; below the first element and from the last one on, the one border element at weight 0.
// Whatever `inv` is, 0 <= i0 <= i1 <= n - 1.
__device__ __forceinline__ void rz_axis(int d, double inv, int n, int& i0, int& i1, float& a) {
  const float c = (float)__dsub_rn(__dmul_rn((double)d + 0.5, inv), 0.5);
  const float fl = floorf(c);
  int i = (int)fminf(fmaxf(fl, -1.f), (float)n);                          // (converted inside the int range; a NaN becomes -1)
  a = __fsub_rn(c, fl);
  if (i < 0) {
    i = 0;
    a = 0.f;
  }
  if (i >= n - 1) {
    i = n - 1;
    a = 0.f;
  }
  i0 = i;
  i1 = min(i + 1, n - 1);
}

// the four taps of one plane in OpenCV's order - the horizontal pass on both rows, then the vertical one - every product and sum
// rounded to float on its own
__device__ __forceinline__ float rz_taps(const float* __restrict__ r0, const float* __restrict__ r1, int x0, int x1, float ax0, float ax1,
                                         float ay0, float ay1) {
  const float top = __fadd_rn(__fmul_rn(r0[x0], ax0), __fmul_rn(r0[x1], ax1));
  const float bot = __fadd_rn(__fmul_rn(r1[x0], ax0), __fmul_rn(r1[x1], ax1));
  return __fadd_rn(__fmul_rn(top, ay0), __fmul_rn(bot, ay1));
}

// The MDR loader's DenseSparseAugmentor - bilinear rescale, flow * scale, flips, crop, valid mask - and the training loop's
// cat((old, new), dim=1) and polarity split in one pass: sample blockIdx.y, one lane per output pixel (x fastest, strided over the
// sample's workgroups) over the nF voxel planes and the two flow planes.  A pixel's taps and weights are formed once; a sample that is
// not resized copies its one source pixel.  The flow is (float)((double)value * mul); the mask is decided on the two doubles.
__global__ __launch_bounds__(256) void augment_resize_kernel(const float* __restrict__ vox_old, const float* __restrict__ vox_new,
                                                             const float* __restrict__ flow, float* __restrict__ out,
                                                             float* __restrict__ label_out, float* __restrict__ mask_out, PcGeom g,
                                                             int nF, RzParams a, unsigned* __restrict__ mm, int want_minmax,
                                                             int per_sample) {
  const int b = blockIdx.y;
  const int hw = g.h * g.w;
  const int sy = a.flags[b] & 2 ? -1 : 1, sx = a.flags[b] & 1 ? -1 : 1;
  const bool resized = a.flags[b] & 4;
  const int64_t plane = (int64_t)g.Hs * g.Ws;
  const int n_old = nF - g.bins;                                           // (0 or bins: the old volume's planes come first)
  float* dst = out + (int64_t)b * nF * 2 * hw;
  unsigned nlo = 0u, hi = 0u;                                              // (~min, max) over nothing
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    const int y = p / g.w, x = p % g.w;
    int y0 = a.by[b] + sy * y, x0 = a.bx[b] + sx * x, y1 = y0, x1 = x0;
    float ay = 0.f, ax = 0.f;
    if (resized) {
      rz_axis(y0, a.inv_y[b], g.Hs, y0, y1, ay);
      rz_axis(x0, a.inv_x[b], g.Ws, x0, x1, ax);
    }
    const float ay0 = __fsub_rn(1.f, ay), ax0 = __fsub_rn(1.f, ax);
    const int64_t o0 = (int64_t)y0 * g.Ws, o1 = (int64_t)y1 * g.Ws;
    for (int c = 0; c < nF; ++c) {
      const float* src = c < n_old ? vox_old + ((int64_t)b * g.bins + c) * plane : vox_new + ((int64_t)b * g.bins + c - n_old) * plane;
      const float v = resized ? rz_taps(src + o0, src + o1, x0, x1, ax0, ax, ay0, ay) : src[o0 + x0];
      mi_split_store(v, dst + (int64_t)c * 2 * hw + p, hw, nlo, hi);
    }
    const float* fu = flow + (int64_t)b * 2 * plane;
    const float u = resized ? rz_taps(fu + o0, fu + o1, x0, x1, ax0, ax, ay0, ay) : fu[o0 + x0];
    const float v = resized ? rz_taps(fu + plane + o0, fu + plane + o1, x0, x1, ax0, ax, ay0, ay) : fu[plane + o0 + x0];
    const double du = __dmul_rn((double)u, a.mul_x[b]), dv = __dmul_rn((double)v, a.mul_y[b]);
    label_out[(int64_t)b * 2 * hw + p] = (float)du;
    label_out[(int64_t)b * 2 * hw + hw + p] = (float)dv;
    // ~isinf(u) & ~isinf(v) & (norm > 0): a NaN fails the comparison, and so do two zeros
    const bool on = !isinf(du) && !isinf(dv) && __dadd_rn(__dmul_rn(du, du), __dmul_rn(dv, dv)) > 0.0;
    mask_out[(int64_t)b * hw + p] = on ? 1.f : 0.f;
  }
  if (want_minmax) mi_minmax_commit(nlo, hi, mm + 2 * (per_sample ? b : 0));
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

// Geometry check of sdf_augment_resize_fwd and the kernel's per-sample arguments; false = SDF_E_SHAPE.  Per sample: a scale that is
// finite and positive and a resized size (rh, rw) = rint(Hs scale_y), rint(Ws scale_x) (half to even, as cvRound) - or, not resized,
// the source's own size -, no smaller than the crop, and an origin inside [0, rh - h] x [0, rw - w].  The kernel then addresses rows
// 0 .. rh - 1 of the resized image, and rz_axis keeps every tap inside the source.
bool rz_geom(const SdfAugmentResizeDesc* d, PcGeom& g, RzParams& a) {
  const int lim = 1 << 20;
  if (d->B < 1 || d->B > SDF_AUGMENT_MAX_B || d->bins < 1 || d->Hs < 1 || d->Ws < 1 || d->Hs > lim || d->Ws > lim) return false;
  if (d->crop_h < 1 || d->crop_w < 1) return false;
  g.B = d->B;
  g.bins = d->bins;
  g.Hs = d->Hs;
  g.Ws = d->Ws;
  g.oy = g.ox = 0;                                                         // (per sample: RzParams)
  g.h = d->crop_h;
  g.w = d->crop_w;
  if ((int64_t)2 * g.bins * g.h * g.w >= (1ll << 30) || (int64_t)g.bins * g.Hs * g.Ws >= (1ll << 34)) return false;
  for (int b = 0; b < SDF_AUGMENT_MAX_B; ++b) {
    a.inv_x[b] = a.inv_y[b] = a.mul_x[b] = a.mul_y[b] = 1.0;
    a.by[b] = a.bx[b] = 0;
    a.flags[b] = 0;
    if (b >= g.B) continue;
    const int rh = d->rh[b], rw = d->rw[b];
    const bool hflip = d->flags[b] & 1, vflip = d->flags[b] & 2;
    if (d->resized[b]) {
      const double sx = d->scale_x[b], sy = d->scale_y[b];
      if (!(sx > 0.0) || !(sy > 0.0) || std::isinf(sx) || std::isinf(sy)) return false;
      if ((double)rh != std::nearbyint(g.Hs * sy) || (double)rw != std::nearbyint(g.Ws * sx)) return false;
      a.inv_x[b] = 1.0 / sx;
      a.inv_y[b] = 1.0 / sy;
      a.mul_x[b] = sx;
      a.mul_y[b] = sy;
    } else if (rh != g.Hs || rw != g.Ws) {
      return false;
    }
    if (rh < g.h || rw < g.w || rh > lim || rw > lim) return false;
    if (d->oy[b] < 0 || d->ox[b] < 0 || d->oy[b] > rh - g.h || d->ox[b] > rw - g.w) return false;
    if (hflip) a.mul_x[b] = -a.mul_x[b];
    if (vflip) a.mul_y[b] = -a.mul_y[b];
    a.by[b] = vflip ? rh - 1 - d->oy[b] : d->oy[b];
    a.bx[b] = hflip ? rw - 1 - d->ox[b] : d->ox[b];
    a.flags[b] = (uint8_t)((d->flags[b] & 3) | (d->resized[b] ? 4 : 0));
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
  int rc = 0;
  const int per_sample = d->per_sample != 0, want_minmax = d->norm == 1;
  if (want_minmax && (rc = mi_clear_pairs(mm, per_sample ? g.B : 1, s))) return rc;
  const int hw = g.h * g.w;
  const int64_t cells = (int64_t)g.bins * hw;
  // at most 1024 workgroups in all (one atomic pair each), at least one per sample
  const int64_t cap = 1024 / g.B > 1 ? 1024 / g.B : 1, need = (cells + 255) / 256;
  const dim3 block(256), sgrid((unsigned)(need < cap ? need : cap), g.B);
  SDF_LAUNCH(prepare_split_kernel, sgrid, block, 0, s, d->voxel, d->out, g, mm, want_minmax, per_sample);
  SDF_LAUNCH_CHECK();
  return mi_finish(d->out, d->event_mask, nullptr, g.B, hw, 2 * g.bins, mm, want_minmax, per_sample, d->use_spike_th, d->spike_th, s);
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
  int rc = 0;
  const int per_sample = d->per_sample != 0, want_minmax = d->norm == 1;
  if (want_minmax && (rc = mi_clear_pairs(mm, per_sample ? g.B : 1, s))) return rc;
  const int hw = g.h * g.w;
  const int64_t cells = (int64_t)g.bins * hw;
  // the grid of sdf_prepare_chunk_fwd: at most 1024 workgroups in all (one atomic pair each), at least one per sample
  const int64_t cap = 1024 / g.B > 1 ? 1024 / g.B : 1, need = (cells + 255) / 256;
  const dim3 block(256), sgrid((unsigned)(need < cap ? need : cap), g.B);
  SDF_LAUNCH(augment_split_kernel, sgrid, block, 0, s, d->voxel, d->label, d->valid, d->drop_u, d->out, d->label_out, d->mask_out, g, a, mm,
             want_minmax, per_sample, d->valid_is_u8 != 0, (uint64_t)d->seed, (uint64_t)d->offset);
  SDF_LAUNCH_CHECK();
  return mi_finish(d->out, d->event_mask, d->mask_events ? d->mask_out : nullptr, g.B, hw, 2 * g.bins, mm, want_minmax, per_sample,
                   d->use_spike_th, d->spike_th, s);
}

extern "C" int64_t sdf_augment_resize_workspace_bytes(int B) { return sdf_augment_chunk_workspace_bytes(B); }

extern "C" int sdf_augment_resize_fwd(const SdfAugmentResizeDesc* d, void* stream) {
  if (!d || !d->scale_x || !d->scale_y) return SDF_E_NULL;                 // (the geometry check reads the scales)
  PcGeom g;
  RzParams a;
  if (!rz_geom(d, g, a)) return SDF_E_SHAPE;                               // every sample's window lies inside its resized image
  if (d->norm < 0 || d->norm > 1) return SDF_E_DTYPE;                      // 0 none | 1 min-max ("std" stays the torch function's)
  if (d->num_chunks < 1 || d->num_chunks > 2) return SDF_E_DTYPE;          // data.num_chunks: the new volume, or old | new
  for (int b = 0; b < g.B; ++b)
    if (d->flags[b] & ~3) return SDF_E_DTYPE;                              // bit 0 horizontal, bit 1 vertical
  if (!d->vox_new || !d->flow || !d->out || !d->label_out || !d->mask_out || !d->workspace) return SDF_E_NULL;
  if (d->num_chunks == 2 && !d->vox_old) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)8 * d->B) return SDF_E_SHAPE;
  if (!sdf_aligned(d->vox_old, 4) || !sdf_aligned(d->vox_new, 4) || !sdf_aligned(d->flow, 4) || !sdf_aligned(d->out, 4) ||
      !sdf_aligned(d->label_out, 4) || !sdf_aligned(d->mask_out, 4) || !sdf_aligned(d->event_mask, 4) || !sdf_aligned(d->workspace, 8))
    return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  unsigned* mm = static_cast<unsigned*>(d->workspace);
  int rc = 0;
  const int per_sample = d->per_sample != 0, want_minmax = d->norm == 1;
  if (want_minmax && (rc = mi_clear_pairs(mm, per_sample ? g.B : 1, s))) return rc;
  const int hw = g.h * g.w, nF = d->num_chunks * g.bins;
  // a lane per output pixel; as its siblings at most 1024 workgroups in all (one atomic pair each), at least one per sample
  const int cap = 1024 / g.B > 1 ? 1024 / g.B : 1, need = (hw + 255) / 256;
  SDF_LAUNCH(augment_resize_kernel, dim3((unsigned)(need < cap ? need : cap), g.B), dim3(256), 0, s, d->vox_old, d->vox_new, d->flow, d->out,
             d->label_out, d->mask_out, g, nF, a, mm, want_minmax, per_sample);
  SDF_LAUNCH_CHECK();
  return mi_finish(d->out, d->event_mask, d->mask_events ? d->mask_out : nullptr, g.B, hw, 2 * nF, mm, want_minmax, per_sample,
                   d->use_spike_th, d->spike_th, s);
}
