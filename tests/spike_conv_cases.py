"""Inputs, float64 references and buffer layouts of tests/test_spike_conv_routes_gpu.py (plain CPU code, no GPU call in here).

Every builder is cached: the routes of the test file share one reference per case, and nothing mutates what a builder returned.

Weights.  The reference multiplies by the weights the planes HOLD, rebuilt here from the format - `held_weights` - so that a format's
rounding is not charged to the kernel:
  1 / 3   bf16 planes, each the round-to-nearest-even bf16 of what the planes before it left (csrc/spike_gemm.hip split_weight_kernel;
          oracle/bf16_planes.py restates the TRUNCATING split of the training kernels, which is another function: not used here)
  2       fp16 hi + lo of scale * w, scale the power of two that puts max |w| into [2^14, 2^15): (hi + lo) / scale
  "i8"    balanced base-256 digits of rint(w / col_scale): (d2 * 65536 + d1 * 256 + d0) * col_scale (csrc/spike_conv_wres.hip)
The GPU file asserts that these are the device's planes bit for bit.

Two kinds of operands:
  exact   at most one spike per pixel (the channel chosen per pixel), so a window holds at most 9 ones; weights exact in the format:
          G.weights(..., exact=True) for 16-bit planes (every partial sum a multiple of 2^-19 below 2^5), multiples of 2^-10 below 1/8
          for digit planes (every partial sum a multiple of 2^-10 below 2^1.2): fp32 accumulation is exact in any order and the
          float64 result IS the fp32 result.  Those digit weights are q = k * 2^16 against the row scale 2^-26: only the top digit
          holds bits.  exact = "fine" is a second set on a grid of 2^-26 whose three digits all carry bits (see `weights`)
  random  spikes at rate 0.3, |w| <= 0.3; one image is silent; with BN alpha in (0.5, 1.5), every fifth entry negative, and one
          output column has alpha = beta = 0.  mag = |alpha| conv(A, |W|) + |beta| + |resid| per element.

The operand A is a slice of a larger buffer: one guard image of all ones in front of it and one behind it, the images of the call
contiguous between them as the ABI requires.  A tap outside an image that is not read as zero then adds a whole weight to the result.
"""
import functools
import math

import numpy as np
import torch

import spike_gemm_cases as G
from oracle import neuron_ref as R
from oracle import sdformer_oracle as O
from sdformerflow_amd.synthetic import synth_uniform as rnd

GUARD = G.GUARD
V_TH, TAU = G.V_TH, G.TAU
TAPS3 = (3, 3, (-1, 0, 1), (-1, 0, 1))           # (KH, KW, dy, dx) of the 3x3 / pad 1 convolution
FORMATS = (1, 2, 3, "i8")


# ---------------------------------------------------------------------------------------------------- weights as the planes hold them
def digit_planes(W):
    """(N, K) fp32 -> (int8 planes (3, N, K), col_scale (N,) fp32): sdf_split_weight_i8x3 restated."""
    mx = W.abs().max(1).values.numpy().astype(np.float32)
    f, ex = np.frexp(mx)                                                   # mx = f * 2^ex, f in [0.5, 1); mx = 0: f = 0, ex = 0
    ex = np.maximum(ex, -100)
    bits = np.where(f <= np.float32(0.996), 23, 22)
    scale = np.ldexp(np.float64(1.0), ex - bits)
    q = np.rint(W.numpy().astype(np.float64) / scale[:, None]).astype(np.int64)     # the quotient is exact: rintf's ties-to-even
    d0 = ((q + 128) & 255) - 128
    q = (q - d0) >> 8
    d1 = ((q + 128) & 255) - 128
    d2 = (q - d1) >> 8
    assert np.abs(d2).max() <= 127
    return torch.from_numpy(np.stack([d0, d1, d2]).astype(np.int8)), torch.from_numpy(scale.astype(np.float32))


def f16_scale(W):
    mx = float(W.abs().max())
    return 2.0 ** (14 - math.floor(math.log2(mx))) if mx > 0 else 1.0


def plane_bits(W, fmt):
    """The 16-bit planes (fmt, N, K) int16 of hip.split_weight(W, fmt), rebuilt on the CPU."""
    if fmt == 2:
        w = W * f16_scale(W)                                               # exact
        hi = w.half()
        return torch.stack([hi, (w - hi.float()).half()]).view(torch.int16)
    r, planes = W.clone(), []
    for _ in range(fmt):
        h = r.bfloat16()
        planes.append(h)
        r = r - h.float()                                                  # exact: the residual fits fp32
    return torch.stack(planes).view(torch.int16)


def held_weights(W, fmt):
    """(N, K) float64: the weights a kernel multiplies by when it is given the planes of W in format `fmt`."""
    if fmt == "i8":
        d, sc = digit_planes(W)
        d = d.double()
        return (d[2] * 65536 + d[1] * 256 + d[0]) * sc.double()[:, None]
    p = plane_bits(W, fmt)
    if fmt == 2:
        return p.view(torch.float16).double().sum(0) / f16_scale(W)
    return p.view(torch.bfloat16).double().sum(0)


@functools.lru_cache(maxsize=None)
def weights(N, K, fmt, exact):
    """(N, K) fp32 in (ky, kx, cin) K order.  The 2- and 3-plane formats and the digits share the random matrix."""
    if exact == "fine":
        # digit planes on a finer grid, so that all three digits carry bits: column 0 of every row is 127 / 1024, which pins the row
        # scale to 2^-26; every other weight is a multiple of 2^-26 below 2^-6.  A window holds column 0 at most once: every partial
        # sum is a multiple of 2^-26 below 2^-3 + 8 * 2^-6 = 2^-2 - 24 bits
        assert fmt == "i8"
        g = np.random.Generator(np.random.PCG64(5200 + 7 * N + K))
        W = torch.from_numpy((g.integers(-2 ** 20 + 1, 2 ** 20, (N, K)) * 2.0 ** -26).astype(np.float32))
        W[:, 0] = 127.0 / 1024.0
        return W
    if exact and fmt == "i8":
        g = np.random.Generator(np.random.PCG64(5100 + 7 * N + K))
        W = torch.from_numpy((g.integers(-127, 128, (N, K)) / 1024.0).astype(np.float32))
        W[0, 0] = 127.0 / 1024.0
        return W
    return G.weights(N, K, fmt == 1, exact)


@functools.lru_cache(maxsize=None)
def held(N, K, fmt, exact):
    return held_weights(weights(N, K, fmt, exact), fmt)


# ---------------------------------------------------------------------------------------------------- operands and the reference
def out_size(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


@functools.lru_cache(maxsize=None)
def images(imgs, H, W, Cin, exact, seed=0, cin_used=None):
    """(imgs + 2, H, W, Cin) u8: the guard image of ones, the spike images of the call, the guard image of ones."""
    buf = torch.ones((imgs + 2, H, W, Cin), dtype=torch.uint8)
    cu = cin_used or Cin
    A = torch.zeros((imgs, H, W, Cin), dtype=torch.uint8)
    if exact:
        g = np.random.Generator(np.random.PCG64(5300 + 3 * imgs + H + 5 * W + Cin + seed))
        ch = torch.from_numpy(g.integers(0, cu, (imgs, H, W)))
        on = torch.from_numpy(g.random((imgs, H, W)) < 0.9)
        A.scatter_(3, ch.unsqueeze(3), on.to(torch.uint8).unsqueeze(3))    # at most one spike per pixel
    else:
        A[..., :cu] = G.spikes((imgs, H, W, cu), 5400 + 3 * imgs + H + 5 * W + Cin + seed)
        if imgs > 1:
            A[imgs // 2] = 0                                               # the silent image
    buf[1:imgs + 1] = A
    return buf


def tap_conv(A, Wm, taps, stride, OH, OW):
    """out[i, y, x, :] = sum_(a, b) A[i, stride y + dy[a], stride x + dx[b], :] @ Wm[:, tap (a, b)]^T in float64, zero outside the image.
    A (imgs, H, W, Cin) u8, Wm (N, KH KW Cin) float64 -> (imgs OH OW, N)."""
    KH, KW, dy, dx = taps
    imgs, H, W, Cin = A.shape
    Ad = A.double()
    y = torch.zeros((imgs, OH, OW, Wm.shape[0]), dtype=torch.float64)

    def span(n_out, n_in, d):                                              # outputs o with 0 <= stride o + d < n_in
        lo = max(0, -(d // stride)) if d < 0 else 0
        hi = min(n_out, (n_in - 1 - d) // stride + 1)
        return lo, hi
    for a in range(KH):
        for b in range(KW):
            (y0, y1), (x0, x1) = span(OH, H, dy[a]), span(OW, W, dx[b])
            if y1 <= y0 or x1 <= x0:
                continue
            sub = Ad[:, stride * y0 + dy[a]:stride * (y1 - 1) + dy[a] + 1:stride, stride * x0 + dx[b]:stride * (x1 - 1) + dx[b] + 1:stride]
            y[:, y0:y1, x0:x1] += sub @ Wm[:, (a * KW + b) * Cin:(a * KW + b + 1) * Cin].t()
    return y.reshape(imgs * OH * OW, -1)


def bn(N, seed):
    """(alpha, beta): alpha in (0.5, 1.5) with every fifth entry negative, column N // 3 has alpha = beta = 0."""
    alpha, beta = rnd((N,), seed + 1, 0.5, 1.5), rnd((N,), seed + 2, -0.2, 0.2)
    alpha[2::5] *= -1.0
    alpha[N // 3] = beta[N // 3] = 0.0
    return alpha, beta


FLAGS = {"plain": (), "bn": ("bn",), "res_sep": ("res_sep",), "res_in": ("bn", "res_in"), "map": ("map",), "all": ("bn", "res_sep", "map")}


def _epilogue(c, y, mag, M, N, f, seed, dst=None):
    """BN -> row map -> residual on (M, N) float64 y / mag; fills the case dict with what G.f32_layout reads."""
    c.update(alpha=None, beta=None, resid=None)
    if "bn" in f:
        c["alpha"], c["beta"] = bn(N, seed)
        y, mag = y * c["alpha"].double() + c["beta"].double(), mag * c["alpha"].double().abs() + c["beta"].double().abs()
    rows = M + 50 if "map" in f else M
    if dst is None:
        dst = torch.arange(M)
        if "map" in f:                                                     # a permutation into a larger buffer, every seventh row dropped
            dst = torch.randperm(rows, generator=torch.Generator().manual_seed(seed))[:M]
            dst[::7] = -1
    else:
        rows = c["rows"]
    if "res_in" in f or "res_sep" in f:
        c["resid"] = rnd((rows, N), seed + 4, -1.0, 1.0)
        r = c["resid"].double()[dst.clamp(min=0)]
        y, mag = y + r, mag + r.abs()
    c.update(y=y, mag=mag, dst=dst, rows=rows, flags=f, M=M, N=N)
    return c


@functools.lru_cache(maxsize=None)
def f32_case(imgs, H, W, Cin, N, fmt, stride=1, feat="plain", exact=False):
    """One 3x3 / pad 1 convolution with the fp32 epilogue."""
    OH, OW = out_size(H, W, stride)
    K = 9 * Cin
    buf = images(imgs, H, W, Cin, exact)
    A = buf[1:imgs + 1]
    Wh = held(N, K, fmt, exact)
    c = {"imgs": imgs, "H": H, "W": W, "Cin": Cin, "OH": OH, "OW": OW, "stride": stride, "taps": TAPS3, "abuf": buf, "wkey": (N, K, fmt, exact)}
    y, mag = tap_conv(A, Wh, TAPS3, stride, OH, OW), tap_conv(A, Wh.abs(), TAPS3, stride, OH, OW)
    return _epilogue(c, y, mag, imgs * OH * OW, N, FLAGS[feat], 5600 + 3 * imgs + 5 * H + W + N + Cin)


# ---------------------------------------------------------------------------------------------------- transposed-convolution classes
DECONV_TAPS = {0: [(0, 1)], 1: [(0, 2), (1, 0)]}      # output parity -> [(input offset, kernel index)] (engine.deconv_classes)


@functools.lru_cache(maxsize=None)
def deconv_weight(Cin, Cout):
    return rnd((Cin, Cout, 3, 3), 5700 + Cin + Cout, -0.3, 0.3)


@functools.lru_cache(maxsize=None)
def deconv_case(imgs, H, W, Cin, cp, N, fmt, drop=True):
    """The four output-parity classes of ConvTranspose2d(3, 2, 1, 1) on Cin channels padded to cp, stride-1 convolutions of 1 or 2 taps
    a side whose rows a row map scatters into the (imgs, 2H, 2W) output; with `drop` every seventh row of each map is dropped (-1).
    -> dict(abuf, w, classes = [dict(taps, K, Wm fp32 (N, K), dst, y, mag)], rows)."""
    w = deconv_weight(Cin, N)
    buf = images(imgs, H, W, cp, False, seed=17, cin_used=Cin)
    A = buf[1:imgs + 1]
    i, yy, xx = torch.arange(imgs).view(-1, 1, 1), torch.arange(H).view(1, -1, 1), torch.arange(W).view(1, 1, -1)
    classes = []
    for py in (0, 1):
        for px in (0, 1):
            ty, tx = DECONV_TAPS[py], DECONV_TAPS[px]
            wk = torch.zeros((N, len(ty), len(tx), cp))
            for a, (_, ky) in enumerate(ty):
                for b, (_, kx) in enumerate(tx):
                    wk[:, a, b, :Cin] = w[:, :, ky, kx].t()
            Wm = wk.reshape(N, -1)
            if fmt == 1:
                Wm = Wm.bfloat16().float()
            taps = (len(ty), len(tx), tuple(t[0] for t in ty), tuple(t[0] for t in tx))
            Wh = held_weights(Wm, fmt)
            dst = ((i * 2 * H + 2 * yy + py) * 2 * W + 2 * xx + px).reshape(-1)
            full = dst.clone()
            if drop:
                dst[py + 2 * px::7] = -1
            classes.append({"taps": taps, "K": Wm.shape[1], "Wm": Wm, "dst": dst, "full": full, "y": tap_conv(A, Wh, taps, 1, H, W),
                            "mag": tap_conv(A, Wh.abs(), taps, 1, H, W)})
    return {"imgs": imgs, "H": H, "W": W, "Cin": Cin, "cp": cp, "N": N, "abuf": buf, "w": w, "classes": classes, "rows": imgs * 4 * H * W}


def class_case(dc, k, feat="map"):
    """Class k of a deconv_case as a case of its own (its row map, optionally BN and a separate residual)."""
    cl = dc["classes"][k]
    c = {"imgs": dc["imgs"], "H": dc["H"], "W": dc["W"], "Cin": dc["cp"], "OH": dc["H"], "OW": dc["W"], "stride": 1, "taps": cl["taps"],
         "abuf": dc["abuf"], "rows": dc["rows"]}
    return _epilogue(c, cl["y"], cl["mag"], dc["imgs"] * dc["H"] * dc["W"], dc["N"], FLAGS[feat], 5800 + k, dst=cl["dst"])


def union_layout(dc, alpha, beta):
    """The guarded output of all four classes in one buffer (BN alpha / beta applied): G.f32_layout's dict."""
    N, rows = dc["N"], dc["rows"]
    shape = (GUARD + rows + GUARD, N)
    init = torch.full(shape, float("nan"))
    written, ref, mag = torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    for cl in dc["classes"]:
        keep = cl["dst"] >= 0
        at = GUARD + cl["dst"][keep]
        assert not written[at].any()
        written[at] = True
        ref[at] = cl["y"][keep] * alpha.double() + beta.double()
        mag[at] = cl["mag"][keep] * alpha.double().abs() + beta.double().abs()
    return {"init": init, "written": written, "ref": ref, "mag": mag}


# ---------------------------------------------------------------------------------------------------- fused neuron
KINDS = G.KINDS
# (no case needed another seed to keep the REFERENCE's own decisions under the cap on ambiguous ones: the CPU test of the routes file
# asserts the cap for every case)


def positions(T, B, n, order):
    """(pos_count, pos_inner, pos_ostride, t_stride) of images in (t, b) order - index t B + b - or in (b, t) order - index b T + t."""
    return (B * n, B * n, 0, B * n) if order == "tb" else (B * n, n, T * n, n)


def to_steps(rows, T, B, order):
    """(imgs n, N) in image order -> (T, B n, N)."""
    N = rows.shape[-1]
    if order == "tb":
        return rows.reshape(T, -1, N)
    return rows.reshape(B, T, -1, N).permute(1, 0, 2, 3).reshape(T, -1, N)


@functools.lru_cache(maxsize=None)
def _sn_conv(T, B, H, W, Cin, N, fmt, stride, seed):
    """conv -> BN of a fused case, shared by its kinds, orders and forms: (buffer, y, mag) in image-row order, alpha, beta."""
    OH, OW = out_size(H, W, stride)
    buf = images(T * B, H, W, Cin, False, seed=seed)
    A = buf[1:T * B + 1]
    Wh = held(N, 9 * Cin, fmt, False)
    alpha, beta = bn(N, seed)
    y = tap_conv(A, Wh, TAPS3, stride, OH, OW) * alpha.double() + beta.double()
    mag = tap_conv(A, Wh.abs(), TAPS3, stride, OH, OW) * alpha.double().abs() + beta.double().abs()
    return buf, y, mag, alpha, beta


@functools.lru_cache(maxsize=None)
def sn_case(T, B, H, W, Cin, N, fmt, stride, kind, order, resid=False):
    """conv -> BN (-> + residual) -> neuron `kind` over T steps.  x = the float64 pre-activation (T, B n, N) cast to fp32, mag the same
    shape, y64 the float64 membrane input in image-row order."""
    OH, OW = out_size(H, W, stride)
    n, imgs, K = OH * OW, T * B, 9 * Cin
    seed = 5900 + 11 * T + 3 * B + 5 * H + W + N + Cin
    buf, y, mag, alpha, beta = _sn_conv(T, B, H, W, Cin, N, fmt, stride, seed)
    r = None
    if resid:
        r = rnd((imgs * n, N), seed + 4, -1.0, 1.0)
        y, mag = y + r.double(), mag + r.double().abs()
    x = to_steps(y, T, B, order).float().contiguous()
    neuron, v_reset = KINDS[kind]
    Wn, bnn = rnd((T, T), seed + 5, -0.5, 0.5) + 0.5 * torch.eye(T), torch.full((T,), -0.1)
    delta = G.DELTA_ULPS * 2.0 ** -23 * max(float(x.double().pow(2).mean().sqrt()), V_TH)
    return {"T": T, "B": B, "imgs": imgs, "H": H, "W": W, "Cin": Cin, "OH": OH, "OW": OW, "N": N, "stride": stride, "taps": TAPS3, "abuf": buf,
            "wkey": (N, K, fmt, False), "alpha": alpha, "beta": beta, "resid": r, "y64": y, "mag": mag, "x": x, "delta": delta, "order": order,
            "pos": positions(T, B, n, order), "neuron": neuron, "v_reset": v_reset, "v_th": V_TH, "psn_w": Wn, "psn_b": bnn,
            "ncfg": O.NeuronCfg(neuron, V_TH, v_reset, TAU, T), "sd": {"w.weight": Wn, "w.bias": bnn}}


def sn_reference(c, x=None):
    """The reference neuron's spikes (T, B n, N) for a case's x (or for the membrane a kernel wrote, same shape)."""
    return R.neuron_ref(c["x"] if x is None else x, c["neuron"], TAU, c["v_th"], c["v_reset"], psn_w=c["psn_w"], psn_b=c["psn_b"])


def sn_report(c, got):
    return O.delta_consistent(c["x"], got.float(), c["ncfg"], c["sd"], "w.", c["delta"])
