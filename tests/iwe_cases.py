"""The image of warped events restated in numpy (the specification: csrc/event_iwe.hip's header), the event recipes
of test_event_iwe_cpu.py / test_event_iwe_gpu.py and the Flow Warp Loss from integer sums.

Every operation of `restate` is a separately rounded fp32 operation (numpy's ufuncs do not contract), a cell's sum is formed by
np.add.at - unbuffered and sequential - one pass after the other, so its bits are the definition's."""
import math

import numpy as np

f32 = np.float32


def restate(x, y, t, p, flow, crop_origin=(0, 0), scale=1.0, t_ref=1.0, window=(0.0, 1.0), mode="bilinear"):
    """One list: x, y (sensor coordinates), t (list order), p as fp32 arrays, flow (2, h, w) fp32 on the window at `crop_origin`
    -> the image (2, h, w) fp32."""
    x, y, t, p = (np.ascontiguousarray(a, dtype=f32) for a in (x, y, t, p))
    flow = np.ascontiguousarray(flow, dtype=f32)
    _, h, w = flow.shape
    oy, ox = crop_origin
    out = np.zeros(2 * h * w, dtype=f32)
    if t.size == 0:
        return out.reshape(2, h, w)
    a, b, scale, t_ref = f32(window[0]), f32(window[1]), f32(scale), f32(t_ref)
    with np.errstate(all="ignore"):
        tn = (t - t[0]) / (t[-1] - t[0])
        keep = (tn >= a) & (tn <= b)                                           # (a NaN fails)
        tau = (tn - a) / (b - a)
        fx, fy = np.floor(x + f32(0.5)), np.floor(y + f32(0.5))
        keep &= (fx >= ox) & (fx < ox + w) & (fy >= oy) & (fy < oy + h)
        xi, yi = np.where(keep, fx, ox).astype(np.int64) - ox, np.where(keep, fy, oy).astype(np.int64) - oy
        u, v = scale * flow[0, yi, xi], scale * flow[1, yi, xi]
        keep &= np.isfinite(u) & np.isfinite(v)
        d = t_ref - tau
        xw, yw = (x - f32(ox)) + d * u, (y - f32(oy)) + d * v
        ch = np.where(p > 0, 0, 1)
        if mode == "nearest":
            corners = [(np.rint(xw), np.rint(yw))]
        else:
            x0, y0 = np.floor(xw), np.floor(yw)
            corners = [(x0 + f32(dx), y0 + f32(dy)) for dx in (0, 1) for dy in (0, 1)]         # dx outer, dy inner
        for xc, yc in corners:
            ok = keep & (xc >= 0) & (xc < w) & (yc >= 0) & (yc < h)                            # (-0 >= 0)
            wgt = np.ones_like(xw) if mode == "nearest" else (f32(1) - np.abs(xc - xw)) * (f32(1) - np.abs(yc - yw))
            index = (ch * h + np.where(ok, yc, 0).astype(np.int64)) * w + np.where(ok, xc, 0).astype(np.int64)
            np.add.at(out, index[ok], wgt[ok].astype(f32))
    return out.reshape(2, h, w)


def int_stats(image):
    """(sum, sum of squares) of the channel sum of a nearest image (2, h, w), as Python integers."""
    c = np.asarray(image, dtype=np.float64).sum(0)
    assert np.array_equal(c, np.rint(c))
    c = c.astype(np.int64).reshape(-1)
    return int(c.sum()), int((c * c).sum())


def variance(s1, s2, n):
    """The unbiased variance over n pixels from their sum and sum of squares, in fp64 (the form of loss/flow_warp.py)."""
    return (float(s2) - float(s1) * float(s1) / n) / (n - 1)


def fwl(x, y, t, p, flow, **kw):
    """The Flow Warp Loss of one list from integer sums: var(nearest image warped by the flow) / var(the same with scale 0)."""
    n = flow.shape[1] * flow.shape[2]
    scale = kw.pop("scale", 1.0)
    vs = variance(*int_stats(restate(x, y, t, p, flow, scale=scale, mode="nearest", **kw)), n)
    vz = variance(*int_stats(restate(x, y, t, p, flow, scale=0.0, mode="nearest", **kw)), n)
    return vs / vz if vz != 0 else math.nan


DOTS_WINDOW = (32, 40)
DOTS_FLOW = (6.0, -3.0)


def moving_dots(seed=5, dots=200, per_dot=40):
    """200 dots that start uniformly in an 8-pixel inset of a 32 x 40 window and move by (6, -3) pixels over the list; 40 events each
    at uniform times, on the integer pixel rint(start + t (6, -3)).  Returns the time-ordered events and the constant true flow."""
    h, w = DOTS_WINDOW
    r = np.random.default_rng(seed)
    sx, sy = r.uniform(8, w - 8, dots), r.uniform(8, h - 8, dots)
    t = r.uniform(0, 1, (dots, per_dot))
    x, y = np.rint(sx[:, None] + t * DOTS_FLOW[0]), np.rint(sy[:, None] + t * DOTS_FLOW[1])
    pol = r.integers(0, 2, (dots, per_dot))
    order = np.argsort(t.reshape(-1), kind="stable")
    ev = {k: v.reshape(-1)[order].astype(f32) for k, v in (("x", x), ("y", y), ("t", t), ("p", pol))}
    flow = np.empty((2, h, w), dtype=f32)
    flow[0], flow[1] = DOTS_FLOW
    return ev, flow


PARITY_SENSOR = (40, 52)
PARITY_CROP = (32, 40)
FLOW_BLOCK = ((8, 16), (4, 16))                  # window rows, columns where the flow is exactly (2, 1)
HOT = ((17, 21, 300), (17, 22, 70))            # (window row, window column, events): neighbours of one row, so lanes of one wave


def parity_events(origin, n=20000, seed=11, ticks=500):
    """n time-ordered events over and around the 40 x 52 sensor for the window at `origin`: fractional coordinates from -1.5 to half a
    pixel past the far edges, 500 ticks (many equal timestamps), a third of the events on integer pixels, the events of the quarter
    ticks on integer pixels of the flow's (2, 1) block (warped coordinates that are exact integers and exact halves), 300 + 70 events
    of one polarity on two neighbouring pixels."""
    H, W = PARITY_SENSOR
    oy, ox = origin
    r = np.random.default_rng(seed)
    x, y = r.uniform(-1.5, W + 0.5, n), r.uniform(-1.5, H + 0.5, n)
    whole = r.permutation(n)[:n // 3]
    x[whole], y[whole] = np.floor(x[whole]), np.floor(y[whole])
    p = r.integers(0, 2, n).astype(np.float64)
    at = 0
    idx = r.permutation(n)
    for row, col, count in HOT:
        sel = idx[at:at + count]
        x[sel], y[sel], p[sel] = col + ox, row + oy, 1.0
        at += count
    t = np.sort(r.integers(0, ticks, n)).astype(f32)
    t[0], t[-1] = 0, ticks
    quarter = np.flatnonzero(np.isin(t, (ticks / 4, ticks / 2, 3 * ticks / 4)))               # tau 0.25 | 0.5 | 0.75 on the whole window
    (r0, r1), (c0, c1) = FLOW_BLOCK
    x[quarter], y[quarter] = r.integers(c0, c1, quarter.size) + ox, r.integers(r0, r1, quarter.size) + oy
    return {"x": x.astype(f32), "y": y.astype(f32), "t": t, "p": p.astype(f32)}


def parity_flow(seed=12):
    """(2, 32, 40): values that carry events out of the window, a block of (2, 1) (with tau 0.5 | 0.75 and integer pixels: exact
    integers and halves), a small constant flow under the hot pixels (their events stay in one base cell with changing weights),
    NaN and inf pixels."""
    h, w = PARITY_CROP
    r = np.random.default_rng(seed)
    flow = (r.standard_normal((2, h, w)) * 6).astype(f32)
    (r0, r1), (c0, c1) = FLOW_BLOCK
    flow[0, r0:r1, c0:c1], flow[1, r0:r1, c0:c1] = 2.0, 1.0
    for row, col, _ in HOT:
        flow[0, row, col], flow[1, row, col] = 0.25, -0.125
    flow[0, 3, 5], flow[1, 4, 7], flow[0, 20, 30], flow[1, 25, 2] = np.nan, np.inf, -np.inf, np.nan
    return flow
