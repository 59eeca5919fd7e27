"""The three renderings of csrc/flow_render.hip restated in numpy, operation by operation in the precision the kernels use, and the
inputs the CPU and GPU tests share.  tests/test_visualization_cpu.py holds the restatement to the reference's own outputs
(tests/golden/visualization.npz) byte for byte; tests/test_visualization_gpu.py holds the kernels to the restatement."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visualization.npz")
FLOW_FIXTURES = ("rand16x24", "rand5x7", "const", "zero", "hue_edges")
EVENT_FIXTURES = ("poisson", "zero", "sparse", "posmin_eq_max")
# (B, H, W) of the random GPU cases: one workgroup, several samples, rows that are no multiple of 4 floats, many workgroups per sample
RANDOM_SHAPES = ((1, 5, 7), (3, 16, 24), (2, 33, 65), (1, 288, 384))


def flow_image_ref(flow, mask=None):
    """(2, H, W) fp32 [* mask (H, W)] -> (H, W, 3) u8: hue and magnitude in fp32, value and the colour cases in fp64."""
    f32 = np.float32
    fx, fy = np.asarray(flow[0], f32), np.asarray(flow[1], f32)
    if mask is not None:
        fx, fy = fx * np.asarray(mask, f32), fy * np.asarray(mask, f32)
    mag = np.sqrt(fx * fx + fy * fy)
    assert mag.dtype == f32
    lo = mag.min()
    rng = mag.max() - lo
    h = (np.arctan2(fy, fx) + f32(np.pi)) * f32(1.0 / np.pi / 2.0)
    assert h.dtype == f32 and rng.dtype == f32
    v = (mag - lo).astype(np.float64)
    if rng != 0:
        v = v / np.float64(rng)
    h6 = h.astype(np.float64) * 6.0
    i = h6.astype(np.int64)
    f = h6 - i
    p, q, t = v * 0.0, v * (1.0 - f), v * (1.0 - (1.0 - f))
    case = i % 6
    r = np.choose(case, [v, q, p, p, t, v])
    g = np.choose(case, [t, v, v, q, p, p])
    b = np.choose(case, [p, p, t, v, v, q])
    return (255.0 * np.stack([r, g, b], -1)).astype(np.uint8)


def event_float_image_ref(counts):
    """(2, h, w) fp32 per-polarity sums -> the reference's float image (h, w, 3) = (0, pos', neg') as float64."""
    f32 = np.float32
    pos, neg = np.asarray(counts[0], f32), np.asarray(counts[1], f32)
    pos_min, pos_max = f32(np.percentile(pos, 1)), f32(np.percentile(pos, 99))
    neg_min, neg_max = f32(np.percentile(neg, 1)), f32(np.percentile(neg, 99))
    m = pos_max if pos_max > neg_max else neg_max
    if pos_min != m:
        pos = (pos - pos_min) / (m - pos_min)
    if neg_min != m:
        neg = (neg - neg_min) / (m - neg_min)
    assert pos.dtype == f32 and neg.dtype == f32
    pos, neg = np.clip(pos, 0, 1).astype(np.float64), np.clip(neg, 0, 1).astype(np.float64)
    return np.stack([np.zeros_like(pos), pos, neg], -1)


def event_bytes_of(float_image):
    """The file's RGB bytes of the float image (0, pos', neg'): cv2.imwrite takes image * 255 (fp64) as BGR and rounds each value to the
    nearest integer, halves to even (OpenCV's documented saturate_cast<uchar>(double); np.rint rounds the same way)."""
    return np.rint(float_image[..., ::-1] * 255.0).astype(np.uint8)


def event_image_ref(counts):
    return event_bytes_of(event_float_image_ref(counts))


def event_counts_ref(src, window=None):
    """signed voxel (bins, Hs, Ws) or split input (bins, 2, Hs, Ws) -> (2, h, w) fp32 sums in bin order on the window (oy, ox, h, w)."""
    src = np.asarray(src, np.float32)
    oy, ox, h, w = window if window else (0, 0) + src.shape[-2:]
    src = src[..., oy:oy + h, ox:ox + w]
    pos, neg = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for c in range(src.shape[0]):
        if src.ndim == 4:
            pos, neg = pos + src[c, 0], neg + src[c, 1]
        else:
            pos, neg = pos + np.maximum(src[c], 0), neg + np.maximum(-src[c], 0)
    return np.stack([pos, neg])


def submission_ref(flow):
    """(2, H, W) fp32 -> (H, W, 3) u16: (uint16)(f * 128 + 2 ** 15) in fp32, truncated, clamped to the type's range; third channel 0."""
    a = np.asarray(flow, np.float32) * np.float32(128) + np.float32(32768)
    assert a.dtype == np.float32
    a = np.clip(a, 0, 65535).astype(np.int64).astype(np.uint16)
    return np.stack([a[0], a[1], np.zeros_like(a[0])], -1)


def random_flow(B, H, W, seed):
    """Flows of a few pixels with a per-sample scale, so that the samples of a batch have different magnitude ranges."""
    r = np.random.default_rng(seed)
    scale = r.uniform(0.5, 20.0, (B, 1, 1, 1))
    return (r.standard_normal((B, 2, H, W)) * scale).astype(np.float32)


def random_voxel(B, bins, H, W, seed):
    """A signed voxel like the loaders': most cells empty, the rest fractional counts of either sign."""
    r = np.random.default_rng(seed)
    v = r.standard_normal((B, bins, H, W)) * (r.random((B, bins, H, W)) < 0.3) * r.uniform(0.5, 3.0, (B, 1, 1, 1))
    return v.astype(np.float32)


def byte_report(got, want):
    """(largest byte difference, share of differing bytes)"""
    d = np.abs(np.asarray(got, np.int64) - np.asarray(want, np.int64))
    return int(d.max()), float((d != 0).mean())
