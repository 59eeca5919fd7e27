// What was evaluated, as images on the stream, gfx950: flow maps as the reference's colour wheel, flow maps in the DSEC benchmark's
// 16-bit encoding, and the event counts of a sample as the green / red image (reference utils/visualization.py Visualization_DSEC:
// flow_to_image :257-282, the `flow_test` branch of store :198-207, events_to_image :297-341; `vis.store`).
//
// The reference renders on the host with numpy, matplotlib and cv2 after copying every tensor back as fp32.  Here a sample's bytes
// (3 per pixel) are written into a caller's buffer next to the metrics, with no read-back and nothing allocated, so the calls are legal
// inside a captured graph.  Compiled with -ffp-contract=off: every product, sum and quotient below is rounded on its own, in the
// precision numpy uses at that place (fp32 up to the hue and the magnitude, fp64 from the division by the range on).
//
// Flow planes are read by QUADS of 4 consecutive pixels per lane: 16 bytes per plane and lane where the planes of a sample (fx, fy and
// the mask) share their alignment - quad 0 is then the up to 3 pixels in front of the first 16-byte boundary, the last quad the tail -
// and element-wise otherwise, so that nothing outside [base, base + H W) is touched whatever the base's alignment.  The 12 (or 24) bytes
// of a quad's pixels are written by the lane that read them.
//
// Launch sequences: flow image: [set the min / max words] | min / max of the magnitude | render.  submission: one launch.
// event image: stage 0 bin sums | (the caller's percentiles) | stage 1 render.
#include "host_launch.h"

namespace {

constexpr int kFrThreads = 256;

struct FrPlanes {
  const float* fx;
  const float* fy;
  const float* m;
  int hw, head;
  bool vec;
};

struct FrQuad {
  float x[4], y[4];
  int p0, n;                                                // pixels p0 .. p0 + n - 1 of the sample
};

__device__ __forceinline__ FrPlanes fr_planes(const float* flow, const float* mask, int b, int hw) {
  FrPlanes P;
  P.fx = flow + (int64_t)b * 2 * hw;
  P.fy = P.fx + hw;
  P.m = mask ? mask + (int64_t)b * hw : nullptr;
  P.hw = hw;
  const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(P.fx) & 15);
  P.vec = (unsigned)(reinterpret_cast<uintptr_t>(P.fy) & 15) == a && (!P.m || (unsigned)(reinterpret_cast<uintptr_t>(P.m) & 15) == a);
  P.head = P.vec ? (int)(((16u - a) & 15u) >> 2) : 0;       // floats in front of the first 16-byte boundary
  if (P.head > hw) P.head = hw;
  return P;
}

// quad q of the sample: 0 = the head, q >= 1 = pixels head + 4 (q - 1) ..; n = 0 behind the sample's end
__device__ __forceinline__ FrQuad fr_load(const FrPlanes& P, int q) {
  FrQuad Q;
  Q.p0 = q == 0 ? 0 : P.head + 4 * (q - 1);
  const int end = q == 0 ? P.head : min(P.hw, Q.p0 + 4);
  Q.n = max(end - Q.p0, 0);
  float m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) Q.x[k] = Q.y[k] = m[k] = 0.f;
  if (P.vec && q > 0 && Q.n == 4) {
    const float4 vx = *reinterpret_cast<const float4*>(P.fx + Q.p0), vy = *reinterpret_cast<const float4*>(P.fy + Q.p0);
    Q.x[0] = vx.x; Q.x[1] = vx.y; Q.x[2] = vx.z; Q.x[3] = vx.w;
    Q.y[0] = vy.x; Q.y[1] = vy.y; Q.y[2] = vy.z; Q.y[3] = vy.w;
    if (P.m) {
      const float4 vm = *reinterpret_cast<const float4*>(P.m + Q.p0);
      m[0] = vm.x; m[1] = vm.y; m[2] = vm.z; m[3] = vm.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < Q.n) {
        Q.x[k] = P.fx[Q.p0 + k];
        Q.y[k] = P.fy[Q.p0 + k];
        if (P.m) m[k] = P.m[Q.p0 + k];
      }
    }
  }
  if (P.m) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      Q.x[k] = Q.x[k] * m[k];
      Q.y[k] = Q.y[k] * m[k];
    }
  }
  return Q;
}

// np.linalg.norm over the two components in fp32
__device__ __forceinline__ float fr_mag(float fx, float fy) { return sqrtf(fx * fx + fy * fy); }

// grid (tiles, B): the sample's min / max magnitude as bit patterns (mag >= 0: the bits order as the values) into mn[b] / mx[b]
__global__ __launch_bounds__(kFrThreads) void flow_render_minmax_kernel(const float* __restrict__ flow, const float* __restrict__ mask, int hw,
                                                                        unsigned* __restrict__ mn, unsigned* __restrict__ mx) {
  const int b = blockIdx.y;
  const FrPlanes P = fr_planes(flow, mask, b, hw);
  const FrQuad Q = fr_load(P, blockIdx.x * kFrThreads + threadIdx.x);
  unsigned kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < Q.n) {
      const unsigned key = __float_as_uint(fr_mag(Q.x[k], Q.y[k]));
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off));
    kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off));
  }
  constexpr int Wv = kFrThreads / 64;
  __shared__ unsigned r_min[Wv], r_max[Wv];
  if ((threadIdx.x & 63) == 0) {
    r_min[threadIdx.x >> 6] = kmin;
    r_max[threadIdx.x >> 6] = kmax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < Wv; ++w) {
      kmin = min(kmin, r_min[w]);
      kmax = max(kmax, r_max[w]);
    }
    if (kmin <= kmax) {                                     // at least one pixel was seen
      atomicMin(mn + b, kmin);
      atomicMax(mx + b, kmax);
    }
  }
}

// One pixel of flow_to_image: hue and magnitude in fp32, value and matplotlib's hsv_to_rgb (s = 1) in fp64, bytes truncated.
__device__ __forceinline__ void fr_flow_pixel(float fx, float fy, float lo, float range, uint8_t* __restrict__ o) {
  const float kPi = (float)3.14159265358979323846, kInv2Pi = (float)(1.0 / 3.14159265358979323846 / 2.0);
  const float mag = fr_mag(fx, fy);
  const float ang = atan2f(fy, fx) + kPi;
  const float h = ang * kInv2Pi;
  double v = (double)(mag - lo);
  if (range != 0.f) v = v / (double)range;
  const double s = 1.0;
  const double h6 = (double)h * 6.0;
  const int i = (int)h6;
  const double f = h6 - (double)i;
  const double p = v * (1.0 - s);
  const double q = v * (1.0 - s * f);
  const double t = v * (1.0 - (s * (1.0 - f)));
  double r, g, bl;
  switch ((unsigned)i % 6u) {                               // (h == 1: i = 6 is case 0)
    case 0: r = v; g = t; bl = p; break;
    case 1: r = q; g = v; bl = p; break;
    case 2: r = p; g = v; bl = t; break;
    case 3: r = p; g = q; bl = v; break;
    case 4: r = t; g = p; bl = v; break;
    default: r = v; g = p; bl = q; break;
  }
  o[0] = (uint8_t)(int)(255.0 * r);
  o[1] = (uint8_t)(int)(255.0 * g);
  o[2] = (uint8_t)(int)(255.0 * bl);
}

__global__ __launch_bounds__(kFrThreads) void flow_render_image_kernel(const float* __restrict__ flow, const float* __restrict__ mask, int hw,
                                                                       const unsigned* __restrict__ mn, const unsigned* __restrict__ mx,
                                                                       uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const FrPlanes P = fr_planes(flow, mask, b, hw);
  const FrQuad Q = fr_load(P, blockIdx.x * kFrThreads + threadIdx.x);
  const float lo = __uint_as_float(mn[b]), hi = __uint_as_float(mx[b]);
  const float range = hi - lo;
  uint8_t* o = out + ((int64_t)b * hw + Q.p0) * 3;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < Q.n) fr_flow_pixel(Q.x[k], Q.y[k], lo, range, o + 3 * k);
}

// (uint16)(f * 128.f + 32768.f): truncated, clamped to the type's range (NaN: 0)
__device__ __forceinline__ uint16_t fr_sub16(float f) {
  const float p = f * 128.f;
  const float a = p + 32768.f;
  return a != a ? (uint16_t)0 : (uint16_t)(int)fminf(fmaxf(a, 0.f), 65535.f);
}

__global__ __launch_bounds__(kFrThreads) void flow_render_submission_kernel(const float* __restrict__ flow, int hw, uint16_t* __restrict__ out) {
  const int b = blockIdx.y;
  const FrPlanes P = fr_planes(flow, nullptr, b, hw);
  const FrQuad Q = fr_load(P, blockIdx.x * kFrThreads + threadIdx.x);
  uint16_t* o = out + ((int64_t)b * hw + Q.p0) * 3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < Q.n) {
      o[3 * k + 0] = fr_sub16(Q.x[k]);
      o[3 * k + 1] = fr_sub16(Q.y[k]);
      o[3 * k + 2] = (uint16_t)0;
    }
  }
}

struct EvGeom {
  int32_t B, bins, Hs, Ws, oy, ox, h, w, split;
};

// relu as ATen's device clamp_min forms it (prepare_chunk.hip): NaN stays
__device__ __forceinline__ float ev_relu(float v) { return v != v ? v : fmaxf(v, 0.f); }

// grid (tiles, B), one lane per pixel of the window: the two polarity sums over the bins, in bin order
__global__ __launch_bounds__(kFrThreads) void flow_render_event_sum_kernel(const float* __restrict__ src, EvGeom g, float* __restrict__ vis) {
  const int b = blockIdx.y, hw = g.h * g.w;
  const int i = blockIdx.x * kFrThreads + threadIdx.x;
  if (i >= hw) return;
  const int y = i / g.w, x = i - y * g.w;
  const int64_t plane = (int64_t)g.Hs * g.Ws, at = (int64_t)(g.oy + y) * g.Ws + g.ox + x;
  float pos = 0.f, neg = 0.f;
  if (g.split) {
    const float* s = src + (int64_t)b * g.bins * 2 * plane + at;
    for (int c = 0; c < g.bins; ++c) {
      pos = pos + s[(int64_t)(2 * c) * plane];
      neg = neg + s[(int64_t)(2 * c + 1) * plane];
    }
  } else {
    const float* s = src + (int64_t)b * g.bins * plane + at;
    for (int c = 0; c < g.bins; ++c) {
      const float v = s[(int64_t)c * plane];
      pos = pos + ev_relu(v);
      neg = neg + ev_relu(-v);
    }
  }
  vis[(int64_t)b * 2 * hw + i] = pos;
  vis[(int64_t)b * 2 * hw + hw + i] = neg;
}

// events_to_image's normalisation of one polarity in fp32, then the byte cv2.imwrite stores for 255 * x (fp64, halves to even)
__device__ __forceinline__ uint8_t ev_byte(float c, float lo, float m) {
  if (lo != m) c = (c - lo) / (m - lo);
  c = c != c ? c : fminf(fmaxf(c, 0.f), 1.f);
  return (uint8_t)(int)rint((double)c * 255.0);
}

__global__ __launch_bounds__(kFrThreads) void flow_render_event_image_kernel(const float* __restrict__ vis, const float* __restrict__ bounds, int hw,
                                                                             uint8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * kFrThreads + threadIdx.x;
  if (i >= hw) return;
  const float* q = bounds + 4 * b;
  const float pos_min = q[0], pos_max = q[1], neg_min = q[2], neg_max = q[3];
  const float m = pos_max > neg_max ? pos_max : neg_max;
  const float pos = vis[(int64_t)b * 2 * hw + i], neg = vis[(int64_t)b * 2 * hw + hw + i];
  uint8_t* o = out + ((int64_t)b * hw + i) * 3;
  o[0] = ev_byte(neg, neg_min, m);                          // the file's R, G, B = the BGR image (0, pos', neg') read backwards
  o[1] = ev_byte(pos, pos_min, m);
  o[2] = (uint8_t)0;
}

// quads a sample of hw pixels can have (the head, the whole vectors behind it, the tail) in workgroups; 0 = refused geometry
inline int64_t fr_tiles(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1) return 0;
  const int64_t hw = (int64_t)H * W;
  if (hw >= (1ll << 30)) return 0;                          // pixel indices, 3 hw and the quad index stay inside 31 bits
  const int64_t quads = 1 + (hw + 3) / 4;
  return (quads + kFrThreads - 1) / kFrThreads;
}

// geometry check of the event image; false = SDF_E_SHAPE
bool ev_geom(const SdfEventImageDesc* d, EvGeom& g) {
  if (d->B < 1 || d->B > 65535 || d->bins < 1 || d->Hs < 1 || d->Ws < 1 || d->crop_h < 0 || d->crop_w < 0) return false;
  if ((d->crop_h == 0) != (d->crop_w == 0) || d->crop_oy < 0 || d->crop_ox < 0) return false;
  if (d->crop_h == 0 && (d->crop_oy || d->crop_ox)) return false;
  if ((int64_t)d->crop_oy + d->crop_h > d->Hs || (int64_t)d->crop_ox + d->crop_w > d->Ws) return false;      // the window lies inside the source
  g.B = d->B;
  g.bins = d->bins;
  g.Hs = d->Hs;
  g.Ws = d->Ws;
  g.oy = d->crop_oy;
  g.ox = d->crop_ox;
  g.h = d->crop_h ? d->crop_h : d->Hs;
  g.w = d->crop_w ? d->crop_w : d->Ws;
  g.split = d->mode;
  if ((int64_t)g.h * g.w >= (1ll << 30)) return false;
  // the last source float's offset stays inside 60 bits
  return (int64_t)g.Hs * g.Ws < (1ll << 60) / ((int64_t)g.B * g.bins * 2);
}

}  // namespace

extern "C" int64_t sdf_flow_image_workspace_bytes(int B, int H, int W) { return fr_tiles(B, H, W) ? (int64_t)8 * B : 0; }

extern "C" int sdf_flow_image_fwd(const SdfFlowImageDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  const int64_t tiles = fr_tiles(d->B, d->H, d->W);
  if (!tiles) return SDF_E_SHAPE;
  if (!d->flow || !d->out || !d->workspace) return SDF_E_NULL;
  if (d->workspace_bytes < (int64_t)8 * d->B) return SDF_E_SHAPE;
  if (!sdf_aligned(d->flow, 4) || !sdf_aligned(d->mask, 4) || !sdf_aligned(d->workspace, 4)) return SDF_E_ALIGN;
  hipStream_t s = sdf_stream(stream);
  unsigned* mn = static_cast<unsigned*>(d->workspace);
  unsigned* mx = mn + d->B;
  hipError_t e = hipMemsetAsync(mn, 0xFF, (size_t)4 * d->B, s);          // min over nothing
  if (e == hipSuccess) e = hipMemsetAsync(mx, 0, (size_t)4 * d->B, s);   // max over nothing
  if (e != hipSuccess) return (int)e;
  const int hw = d->H * d->W;
  const dim3 grid((unsigned)tiles, d->B), block(kFrThreads);
  SDF_LAUNCH(flow_render_minmax_kernel, grid, block, 0, s, d->flow, d->mask, hw, mn, mx);
  SDF_LAUNCH_CHECK();
  SDF_LAUNCH(flow_render_image_kernel, grid, block, 0, s, d->flow, d->mask, hw, mn, mx, d->out);
  return sdf_launch_rc();
}

extern "C" int sdf_flow_submission_fwd(const SdfFlowSubmissionDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  const int64_t tiles = fr_tiles(d->B, d->H, d->W);
  if (!tiles) return SDF_E_SHAPE;
  if (!d->flow || !d->out) return SDF_E_NULL;
  if (!sdf_aligned(d->flow, 4) || !sdf_aligned(d->out, 2)) return SDF_E_ALIGN;
  SDF_LAUNCH(flow_render_submission_kernel, dim3((unsigned)tiles, d->B), dim3(kFrThreads), 0, sdf_stream(stream), d->flow, d->H * d->W,
             static_cast<uint16_t*>(d->out));
  return sdf_launch_rc();
}

extern "C" int sdf_event_image_fwd(const SdfEventImageDesc* d, void* stream) {
  if (!d) return SDF_E_NULL;
  if (d->mode < 0 || d->mode > 1 || d->stage < 0 || d->stage > 1) return SDF_E_DTYPE;
  EvGeom g;
  if (!ev_geom(d, g)) return SDF_E_SHAPE;
  if (!d->chunk_vis || (d->stage == 0 ? !d->src : (!d->bounds || !d->out))) return SDF_E_NULL;
  if (!sdf_aligned(d->src, 4) || !sdf_aligned(d->chunk_vis, 4) || !sdf_aligned(d->bounds, 4)) return SDF_E_ALIGN;
  const int hw = g.h * g.w;
  const dim3 grid((unsigned)((hw + kFrThreads - 1) / kFrThreads), g.B), block(kFrThreads);
  hipStream_t s = sdf_stream(stream);
  if (d->stage == 0)
    SDF_LAUNCH(flow_render_event_sum_kernel, grid, block, 0, s, d->src, g, d->chunk_vis);
  else
    SDF_LAUNCH(flow_render_event_image_kernel, grid, block, 0, s, d->chunk_vis, d->bounds, hw, d->out);
  return sdf_launch_rc();
}
