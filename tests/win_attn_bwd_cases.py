"""Shared by test_win_attn_bwd_reference_cpu.py and test_win_attn_bwd_routes_gpu.py: the two window-attention backward passes written
out as formulas (no autograd), the per-element magnitude of every result, the d_bias run split of the three kernels that have one, and
the case table.  Importable without a GPU.

`sew_backward` / `ann_backward` evaluate in the dtype of their inputs: float64 is the reference, float32 on the CPU is what pins the
constants KAPPA (test_win_attn_bwd_reference_cpu.py).  With absolute=True the same function returns, per element, the sum of the
absolute values of the terms the result is summed from: |dO| for dO, |bias + mask| for the SEW bias term, and for the ANN
  dP -> |dO| |v|^T,  dS -> P o (|dP| + D_abs),  products with |q^|, |k^|, |dO|,  normalize backward (|dy| + |y| (|y| . |dy|)) / n.
The error of a correct fp32 evaluation is a small multiple of 2^-24 of that magnitude (plus, for the ANN, the rounding of the logits
themselves, which grows with the logit: the high-logit family has its own constants); an error that is a fixed fraction of one TERM -
a key too many in a ragged tile, a window too many in a d_bias run - is orders of magnitude above it wherever it lands, also in a part
of the tensor that is small beside the tensor's largest element.

Layouts.  SEW: q, k, v (T', B_, N1, C) read as the raw head view (B_, nH, N, 32); dO arrives in the forward's output scramble
(B_, nH, T', N1, 32) -> (T', B_, N1, C).  ANN: qkv (rows, 3C) in the activation's row order, gathered into windows through the row map
(-1: a padding token, which reads the pad row and whose output is cropped: dO = 0) and scattered back; d_pad = the padding tokens' sum."""
import functools
import math
import zlib

import torch

from win_attn_large_bwd_cases import guarded, guards_hold, label_mask, py_row_map  # noqa: F401  (re-exported to the two test files)

HD = 32
EPS = 1e-12                                  # F.normalize eps
FLOOR = 1e-30                                # bound (b): kappa * magnitude + FLOOR (P under a -100 mask underflows fp32)
TOL = {"ann": 2e-5, "sew": 1e-5}             # bound (a): max |err| <= TOL * max |ref|, per part


# ------------------------------------------------------------------------------------------------------------------------------ SEW
def sew_dout_heads(dout, nH):
    """dO (T', B_, N1, C) -> (B_, nH, N, 32): the forward's output scramble undone"""
    Tq, B_, N1, _ = dout.shape
    return dout.reshape(Tq, B_, N1, nH, HD).permute(1, 3, 0, 2, 4).reshape(B_, nH, Tq * N1, HD)


def sew_backward(q, k, v, scale, bias, mask, nH, dout, absolute=False):
    """q, k, v (T', B_, N1, C) spikes as floats, scale a float, bias (nH, N, N), mask (nW, N, N) or None, dout (T', B_, N1, C)
    -> dq, dk, dv (T', B_, N1, C), d_bias (nH, N, N); absolute: their magnitudes."""
    Tq, B_, N1, _ = q.shape
    Q, K, V = (t.reshape(B_, nH, Tq * N1, HD) for t in (q, k, v))
    dO = sew_dout_heads(dout, nH)
    bm = bias.unsqueeze(0)
    if mask is not None:
        bm = bm + mask[torch.arange(B_, device=mask.device) % mask.shape[0]].unsqueeze(1)       # bm = bias[g] + mask[b % nW]
    if absolute:
        dO, bm = dO.abs(), bm.abs()
    G1 = V.transpose(-2, -1) @ K
    G3 = Q.transpose(-2, -1) @ dO
    dQ = scale * (dO @ G1)
    dK = scale * (V @ G3.transpose(-2, -1))
    dV = scale * (K @ G3) + bm.transpose(-2, -1) @ dO
    d_bias = (dO @ V.transpose(-2, -1)).sum(0)
    return dQ.reshape(q.shape), dK.reshape(q.shape), dV.reshape(q.shape), d_bias


# ------------------------------------------------------------------------------------------------------------------------------ ANN
def _normalize(x):
    n = x.norm(dim=-1, keepdim=True)
    return x / n.clamp_min(EPS), n


def _normalize_bwd(dy, y, n, absolute):
    """y = x / max(n, eps): dx = (dy - y (y . dy)) / n, or dy / eps below the clamp (which passes no gradient to the norm)"""
    if absolute:
        y = y.abs()
        dx = (dy + y * (y * dy).sum(-1, keepdim=True)) / n.clamp_min(EPS)
    else:
        dx = (dy - y * (y * dy).sum(-1, keepdim=True)) / n.clamp_min(EPS)
    return torch.where(n >= EPS, dx, dy / EPS)


def ann_windows_backward(win, dOw, ls, bias, mask, nH, absolute=False):
    """win (B_, N, 3C), dOw (B_, N, C), ls (nH), bias (nH, N, N), mask (nW, N, N) or None -> dwin (B_, N, 3C), d_scale (nH), d_bias"""
    B_, N, _ = win.shape
    q, k, v = win.reshape(B_, N, 3, nH, HD).permute(2, 0, 3, 1, 4)
    dO = dOw.reshape(B_, N, nH, HD).permute(0, 2, 1, 3)
    qh, nq = _normalize(q)
    kh, nk = _normalize(k)
    lsv = ls.reshape(1, nH, 1, 1)
    S = (qh @ kh.transpose(-2, -1)) * lsv + bias.unsqueeze(0)
    if mask is not None:
        S = S + mask[torch.arange(B_, device=mask.device) % mask.shape[0]].unsqueeze(1)
    P = S.softmax(-1)
    if absolute:
        dO, qa, ka = dO.abs(), qh.abs(), kh.abs()
        dP = dO @ v.abs().transpose(-2, -1)
        dS = P * (dP + (P * dP).sum(-1, keepdim=True))
        d_scale = (dS * (qa @ ka.transpose(-2, -1))).sum((0, 2, 3))
    else:
        qa, ka = qh, kh
        dP = dO @ v.transpose(-2, -1)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        d_scale = (dS * (qh @ kh.transpose(-2, -1))).sum((0, 2, 3))
    dv = P.transpose(-2, -1) @ dO
    dq = _normalize_bwd(lsv * (dS @ ka), qh, nq, absolute)
    dk = _normalize_bwd(lsv * (dS.transpose(-2, -1) @ qa), kh, nk, absolute)
    dwin = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(B_, N, 3 * nH * HD)
    return dwin, d_scale, dS.sum(0)


def ann_backward(qkv, pad, row_map, B_, N, ls, bias, mask, nH, dout, absolute=False):
    """qkv (rows, 3C), pad (3C), row_map (B_ * N) or None (rows window-major), dout (rows, C)
    -> dqkv (rows, 3C), d_pad (3C), d_scale (nH), d_bias (nH, N, N); absolute: their magnitudes."""
    if row_map is None:
        dwin, d_scale, d_bias = ann_windows_backward(qkv.reshape(B_, N, -1), dout.reshape(B_, N, -1), ls, bias, mask, nH, absolute)
        return dwin.reshape(qkv.shape), torch.zeros_like(pad), d_scale, d_bias
    m = row_map.long()
    real, idx = m >= 0, m.clamp_min(0)
    win = torch.where(real[:, None], qkv[idx], pad[None]).reshape(B_, N, -1)
    dOw = torch.where(real[:, None], dout[idx], torch.zeros((), dtype=dout.dtype, device=dout.device)).reshape(B_, N, -1)
    dwin, d_scale, d_bias = ann_windows_backward(win, dOw, ls, bias, mask, nH, absolute)
    flat = dwin.reshape(B_ * N, -1)
    dqkv = torch.zeros_like(qkv).index_add_(0, m[real], flat[real])
    return dqkv, flat[~real].sum(0), d_scale, d_bias


# ------------------------------------------------------------------------------------------------- the d_bias run split, restated
DBIAS_TARGET_WG = 2048


def dbias_run(B_, tiles):
    """windows per d_bias run (dbias_run of csrc/win_attn_sew_bwd.hip and csrc/win_attn_large_bwd.hip)"""
    runs = max(1, min(B_, -(-DBIAS_TARGET_WG // tiles)))
    return -(-B_ // runs)


def dbias_runs(B_, tiles):
    return -(-B_ // dbias_run(B_, tiles))


def dbias_tiles(kernel, nH, N):
    """workgroups of one run: sew_bwd_dbias_kernel (16 query rows), win_attn_large_ann_bwd_dbias_kernel (64 x 64 tiles),
    win_attn_large_sew_dbias_kernel (16 query rows x 256 keys)"""
    if kernel == "sew":
        return nH * -(-N // 16)
    if kernel == "large_ann":
        return nH * (-(-N // 64)) ** 2
    assert kernel == "large_sew"
    return nH * -(-N // 16) * -(-N // 256)


# ---------------------------------------------------------------------------------------------------------------------------- cases
# ANN.  Window-major (row_map None): N, B_, nW (0: no mask).  Row-mapped: ws, (B, D, H, W) with H and W no multiples of the window, so
# padding tokens exist; shifted cases carry the shift mask.  high: the forward file's recipe (scale up to 100 with head 0 at exactly 100,
# the clamp's value; bias 16 sigmoid); low: scale 1.5 on every head and |bias| <= 1, so a key wrongly admitted with logit 0 weighs more
# than 1 / (1 + 162 e^2.5) = 5e-4 of a row.
def _wm(N, B_, nW, low=False, nH=3):
    return dict(kind="wm", N=N, B_=B_, nW=nW, low=low, zero_pad=False, nH=nH)


def _rm(ws, shifted, low=False, zero_pad=False, nH=3):
    return dict(kind="rm", ws=ws, grid=(1, 2, 11, 20), shifted=shifted, N=ws[0] * ws[1] * ws[2], low=low, zero_pad=zero_pad, nH=nH)


ANN_CASES = {}
for _n in (1, 16, 81, 128, 192):                 # one tile with one / sixteen tokens (three idle waves), one real token in the last
    ANN_CASES[f"wm{_n}_b3_mask"] = _wm(_n, 3, 3)  # tile, no ragged tile, 12 tiles (dynamic LDS above 64 KiB); 3 windows: below the
    ANN_CASES[f"wm{_n}_b10"] = _wm(_n, 10, 0)     # reduce kernel's eight-wide loop; 10: once through it and two left over
ANN_CASES.update({
    "wm81_b3_mask_low": _wm(81, 3, 3, low=True),
    "rm162_shift": _rm((2, 9, 9), True),
    "rm98_shift": _rm((2, 7, 7), True),
    "rm162_shift_low": _rm((2, 9, 9), True, low=True),
    "rm98_shift_low": _rm((2, 7, 7), True, low=True),
    "rm162_zero_pad": _rm((2, 9, 9), False, zero_pad=True),
    "rm162_shift_h12": _rm((2, 9, 9), True, nH=12),
})
ANN_LARGE_CASES = {                              # win_attn_large_ann_bwd_dbias_kernel with more than one window per run
    "wm200_b50": _wm(200, 50, 0),                # 48 tiles: 25 runs of 2
    "wm200_b51_mask": _wm(200, 51, 3),           # 26 runs, the last of 1
    "wm450_b13": _wm(450, 13, 0),                # 192 tiles: 7 runs, the last of 1
    "wm200_b12_mask_h12": _wm(200, 12, 3, nH=12),  # 12 heads (192 tiles: 6 runs of 2)
}

# SEW: Tq, N1, B_, nW (0: no mask), nH
SEW_CASES = {}
for _tq, _n1 in ((1, 1), (1, 45), (1, 65), (2, 64), (2, 81), (2, 96)):
    SEW_CASES[f"w{_tq}x{_n1}"] = (_tq, _n1, 4, 0, 3)
    SEW_CASES[f"w{_tq}x{_n1}_mask"] = (_tq, _n1, 4, 2, 3)
SEW_CASES.update({
    "runs_w2x96_b23_h12_mask": (2, 96, 23, 23, 12),   # 144 tiles: 12 runs of 2, the last of 1
    "runs_w2x81_b101": (2, 81, 101, 0, 3),            # 33 tiles: 51 runs of 2, the last of 1
})
SEW_LARGE_CASES = {                                   # win_attn_large_sew_dbias_kernel with more than one window per run
    "w1x193_b59": (1, 193, 59, 0, 3),                 # 39 tiles: 30 runs, the last of 1
    "w2x225_b13_mask": (2, 225, 13, 13, 3),           # 174 tiles: 7 runs, the last of 1
}
# case -> (which kernel's split, B_, nH, N): the cases that exist for the in-workgroup window loop and its ragged last run
RUNS_CASES = {
    "runs_w2x96_b23_h12_mask": ("sew", 23, 12, 192), "runs_w2x81_b101": ("sew", 101, 3, 162),
    "wm200_b50": ("large_ann", 50, 3, 200), "wm200_b51_mask": ("large_ann", 51, 3, 200), "wm450_b13": ("large_ann", 13, 3, 450),
    "w1x193_b59": ("large_sew", 59, 3, 193), "w2x225_b13_mask": ("large_sew", 13, 3, 450),
}
RAGGED_LAST_RUN = ("runs_w2x96_b23_h12_mask", "runs_w2x81_b101", "wm200_b51_mask", "wm450_b13", "w1x193_b59", "w2x225_b13_mask")


def ann_family(c):
    return "ann_low" if c["low"] else "ann_high"


# kappa of bound (b) per family and part: 8 x the worst per-element ratio |fp32 - fp64| / magnitude of the CPU's fp32 evaluation of the
# formulas above over the family's cases (the large ones included), rounded up to one digit.  The ratios this table was made from
# (test_win_attn_bwd_reference_cpu.py prints them and asserts kappa / 8):
#              dq        dk        dv        d_bias
#   sew        2.94e-7   1.78e-7   3.29e-7   1.18e-7
#   ann_low    6.42e-8   6.77e-8   3.40e-7   1.15e-7
#   ann_high   2.83e-6   7.60e-6   2.56e-5   1.28e-5
# dq / dk / dv include the thirds of d_pad.  The high-logit ratios are the fp32 rounding of logits near 116 (2^-24 * 116 = 6.9e-6 in the
# exponent, so in P), as in the forward.
KAPPA = {
    "sew": {"dq": 3e-6, "dk": 2e-6, "dv": 3e-6, "d_bias": 1e-6},
    "ann_low": {"dq": 6e-7, "dk": 6e-7, "dv": 3e-6, "d_bias": 1e-6},
    "ann_high": {"dq": 3e-5, "dk": 7e-5, "dv": 3e-4, "d_bias": 2e-4},
}


# Salt of every case's generator.  Chosen among a handful so that no worst ratio below sits within 5 % of its kappa / 8 (the rounding up
# to one digit leaves between 6 % and 49 %): the CPU test then does not hang on the last bit of a BLAS.
SEED = "bwd 3 "


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32((SEED + name).encode()))


def _uniform(shape, g, lo, hi):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


@functools.lru_cache(maxsize=None)
def ann_inputs(name):
    """fp32 CPU inputs of an ANN case: dict(qkv, pad, row_map | None, B_, N, ls, bias, mask | None, nH, dout)"""
    c = {**ANN_CASES, **ANN_LARGE_CASES}[name]
    g, nH, N = _gen("ann " + name), c["nH"], c["N"]
    Cc = nH * HD
    if c["kind"] == "wm":
        B_, row_map = c["B_"], None
        rows = B_ * N
        mask = label_mask(c["nW"], N, g) if c["nW"] else None
    else:
        from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw
        B, D, H, W = c["grid"]
        ws = c["ws"]
        ss = tuple(w // 2 for w in ws) if c["shifted"] else (0, 0, 0)
        row_map, B_ = py_row_map(B, D, H, W, ws, ss)
        rows = B * D * H * W
        Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
        mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, torch.device("cpu")).float().contiguous() if c["shifted"] else None
        assert int((row_map < 0).sum()) > 0 and (mask is None or B_ % mask.shape[0] == 0)
    if c["low"]:
        ls, bias = torch.full((nH,), 1.5), _uniform((nH, N, N), g, -1.0, 1.0)
    else:
        ls = torch.exp(torch.clamp(_uniform((nH,), g, 1.5, 5.0), max=math.log(100.0)))
        ls[0] = 100.0
        bias = 16 * torch.sigmoid(_uniform((nH, N, N), g, -2.0, 2.0))
    qkv = torch.randn((rows, 3 * Cc), generator=g)
    pad = torch.zeros(3 * Cc) if c["zero_pad"] else torch.randn(3 * Cc, generator=g)
    dout = torch.randn((rows, Cc), generator=g)
    return dict(qkv=qkv, pad=pad, row_map=row_map, B_=B_, N=N, ls=ls, bias=bias, mask=mask, nH=nH, dout=dout)


@functools.lru_cache(maxsize=None)
def sew_inputs(name):
    """fp32 CPU inputs of a SEW case: dict(q, k, v (spikes as floats), scale (the fp32 value of 32^-0.5), bias, mask | None, nH, dout)"""
    Tq, N1, B_, nW, nH = {**SEW_CASES, **SEW_LARGE_CASES}[name]
    g, N, Cc = _gen("sew " + name), Tq * N1, nH * HD
    q, k, v = ((torch.rand((Tq, B_, N1, Cc), generator=g) < p).float() for p in (0.3, 0.2, 0.25))
    bias = torch.randn((nH, N, N), generator=g)
    mask = label_mask(nW, N, g) if nW else None
    dout = torch.randn((Tq, B_, N1, Cc), generator=g)
    return dict(q=q, k=k, v=v, scale=float(torch.tensor(HD ** -0.5, dtype=torch.float32)), bias=bias, mask=mask, nH=nH, dout=dout)


def cast(inp, dtype, device=None):
    """the floating tensors of an input dict in `dtype` (and everything on `device`)"""
    out = {}
    for k, v in inp.items():
        if torch.is_tensor(v):
            v = v.to(device) if device is not None else v
            v = v.to(dtype) if v.is_floating_point() else v
        out[k] = v
    return out


def ann_eval(inp, absolute=False):
    return ann_backward(inp["qkv"], inp["pad"], inp["row_map"], inp["B_"], inp["N"], inp["ls"], inp["bias"], inp["mask"], inp["nH"],
                        inp["dout"], absolute)


def sew_eval(inp, absolute=False):
    return sew_backward(inp["q"], inp["k"], inp["v"], inp["scale"], inp["bias"], inp["mask"], inp["nH"], inp["dout"], absolute)


def ann_parts(dqkv, d_pad, d_bias):
    """name -> tensors checked together under that part's kappa: the thirds of dqkv and of d_pad, d_bias"""
    Cc = d_pad.numel() // 3
    parts = {}
    for i, p in enumerate(("dq", "dk", "dv")):
        parts[p] = dqkv[:, i * Cc:(i + 1) * Cc]
        parts["d_pad." + p] = d_pad[i * Cc:(i + 1) * Cc]
    parts["d_bias"] = d_bias
    return parts


def kappa_of(family, part):
    return KAPPA[family][part.split(".")[-1]]


def worst_ratio(got, ref, mag):
    """max over elements of (|got - ref| - FLOOR)+ / magnitude: bound (b) holds with kappa exactly where this is <= kappa (an error
    above the floor where the magnitude is 0 gives inf)"""
    if not ref.numel():
        return 0.0
    over = ((got.double() - ref).abs() - FLOOR).clamp_min(0)
    ratio = torch.where(over > 0, over / mag, torch.zeros_like(over))
    assert not torch.isnan(ratio).any()
    return ratio.max().item()
