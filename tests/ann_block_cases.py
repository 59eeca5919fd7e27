"""Shared cases of the one-launch ANN half blocks (csrc/ann_block.hip, csrc/ann_mlp_block.hip): inputs, float64 references of the two
branches, per-element magnitude sums, and a torch emulation of the kernels' documented numerics.  Pure torch on the CPU; used by
test_ann_block_bound_cpu.py (which fixes the tolerance without a kernel) and test_ann_block_parity_gpu.py (which holds the kernels to it).

The branches (reference models/STSwinNet/swin_transformer3D_v2.py):
  attention  proj(softmax(normalize(q) normalize(k)^T * exp(min(logit_scale, ln 100)) + cpb bias (+ mask)) v) + bp, q | k | v = LN(x) Wqkv^T + b,
             over the windows of the row map (pad / roll / partition; a padding token is a zero row behind the norm, :169-205, :272-310);
  MLP        fc2(gelu(fc1(LN(x)))) (:15-34, :312-336).
Both kernels return x + branch; the tests compare (out - x) with the branch, per element, against

  tol * B + 2^-23 |x + branch64| (+ the MLP's GELU term),

  B      the sum of the magnitudes of the terms of the LAST product (attention: sum_j |Wp[c,j]| (sum_k P[t,k] |V[k,j]|) + |bp[c]|;
         MLP: sum_j |W2[c,j]| |H[t,j]| + |b2[c]|) - what an error relative to every term adds up to;
  tol    8 x the worst (|branch32 - branch64| / B) of the case, branch32 the same reference in plain fp32 (test_ann_block_bound_cpu.py);
  2^-23  of the result: the final fp32 addition of the shortcut and the store;
  GELU   1.5e-7 sum_j |W2[c,j]| |hpre[t,j]|: Abramowitz & Stegun 7.1.26's absolute error bound of erf (the kernel header), times
         |x| in x q; the reference's exact erf has no such error.

No term for the fp16 subnormal floor of the lo planes: every Linear weight here is below 0.25 (+-0.15 and +-0.04), so lo = fp16(w - fp16(w))
lies below 2^-14, where fp16 has the fixed spacing 2^-24, and hi + lo misses w by up to 2^-25 absolute (1.5e-6 of a weight of 0.02).
The emulation carries exactly that rounding and stays within tol on every case (test_ann_block_bound_cpu.py), so the allowance
needs no floor term - PROVIDED the matrix pipe consumes subnormal fp16 inputs.  `ftz=True` emulates one that flushes them to zero.
"""
import functools
import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from oracle import sdformer_oracle as O
from sdformerflow_amd.synthetic import synth_uniform as rnd

C, NH, HD, N, CH = 96, 3, 32, 162, 384
WS = (2, 9, 9)
EPS = 1e-5
LOG2E = 1.4426950408889634
LN100 = math.log(100.0)
FACTOR = 8.0                                     # 4: 22 of 24 bits; 2: the lo lo term and v_exp_f32 / v_rcp_f32 at 1 ulp
GELU_ABS = 1.5e-7
ROWS_WG = 192                                    # rows per workgroup of ann_mlp_block_kernel
ATTN_LDS = 2 * 96 * 224 * 2 + 2 * 176 * 96 + 44 * 32 * 16
MLP_LDS = 2 * 2 * 96 * 224


# ------------------------------------------------------------------------------------------------ parameter recipes
def _randn(shape, seed):
    """Standard normal from synth_uniform (Box-Muller), so that every input comes from the one seeded generator."""
    u = rnd((2,) + tuple(shape), seed, 1e-7, 1.0).double()
    return (torch.sqrt(-2.0 * torch.log(u[0])) * torch.cos(2.0 * math.pi * u[1])).float()


def _weight(shape, seed, recipe):
    if recipe == "wide":
        return rnd(shape, seed, -0.15, 0.15)
    return (0.02 * _randn(shape, seed)).clamp(-0.04, 0.04)                       # trunc-normal std 0.02 (swin's Linear init)


def _norm(seed, recipe):
    if recipe == "wide":
        return rnd((C,), seed, 0.5, 1.5), rnd((C,), seed + 1, -0.3, 0.3)
    return rnd((C,), seed, 0.9, 1.1), rnd((C,), seed + 1, -0.02, 0.02)


def _bias(n, seed, recipe):
    return rnd((n,), seed, -0.2, 0.2) if recipe == "wide" else rnd((n,), seed, -0.02, 0.02)


def logit_scale(ls, seed):
    """(NH, 1, 1) raw parameter.  ls10: ln 10 on every head (the model's initial value).  ls100: head 0 beyond the clamp at ln 100,
    the others between e^1.5 and 100."""
    if ls == "ls10":
        return torch.full((NH, 1, 1), math.log(10.0))
    p = rnd((NH, 1, 1), seed, 1.5, LN100)
    p[0] = 5.0
    return p


def row_map_cpu(B, D, H, W, ss):
    """The int32 gather table of pad -> roll(-shift) -> window_partition (swin_transformer3D_v2.py:283-292) on the row indices of a
    (B, D, H, W) feature map, -1 for padding tokens -> ((B_ * N,), B_, (Dp, Hp, Wp)).  hip.window_slice_map builds the same table
    on the device (the GPU test asserts the two equal)."""
    idx = torch.arange(B * D * H * W).view(B, D, H, W)
    pd, ph, pw = (-D) % WS[0], (-H) % WS[1], (-W) % WS[2]
    idx = F.pad(idx, (0, pw, 0, ph, 0, pd), value=-1)
    Dp, Hp, Wp = D + pd, H + ph, W + pw
    if any(ss):
        idx = torch.roll(idx, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    win = idx.view(B, Dp // WS[0], WS[0], Hp // WS[1], WS[1], Wp // WS[2], WS[2]).permute(0, 1, 3, 5, 2, 4, 6).reshape(-1, N)
    return win.reshape(-1).to(torch.int32).contiguous(), win.shape[0], (Dp, Hp, Wp)


# ------------------------------------------------------------------------------------------------ cases
GEOMETRY = {                 # name: (B, D, H, W, shift)
    "flat1": (1, 2, 9, 9, (0, 0, 0)),            # one workgroup: per_xcd = 0
    "flat8": (8, 2, 9, 9, (0, 0, 0)),            # every workgroup id re-dealt over the XCDs, no remainder
    "flat12": (12, 2, 9, 9, (0, 0, 0)),          # 8 re-dealt + 4 not
    "flat17": (17, 2, 9, 9, (0, 0, 0)),          # odd count
    "mask4": (1, 2, 18, 18, (1, 4, 4)),          # 4 windows, 4 mask tables
    "mask12": (2, 2, 18, 27, (1, 4, 4)),         # 12 windows, 6 mask tables: two windows share each
    "pad": (1, 2, 20, 30, (0, 0, 0)),            # 27 x 36 padded: -1 entries inside a wave's 16 tokens
    "padshift": (1, 2, 20, 30, (1, 4, 4)),       # the same, rolled: padding tokens in the middle of windows, and a mask
}
ATTN_CASES = {               # name: (geometry, recipe, logit scale, options)
    "flat1-wide-ls10": ("flat1", "wide", "ls10", ()),
    "flat1-init-ls10": ("flat1", "init", "ls10", ()),
    "flat8-wide-ls10": ("flat8", "wide", "ls10", ()),
    "flat8-init-ls100": ("flat8", "init", "ls100", ()),
    "flat12-init-ls10": ("flat12", "init", "ls10", ()),
    "flat12-wide-ls100": ("flat12", "wide", "ls100", ()),
    "flat17-wide-ls10": ("flat17", "wide", "ls10", ()),
    "flat17-init-ls10": ("flat17", "init", "ls10", ()),
    "mask4-wide-ls10": ("mask4", "wide", "ls10", ()),
    "mask4-init-ls10": ("mask4", "init", "ls10", ()),
    "mask4-wide-ls100": ("mask4", "wide", "ls100", ()),
    "mask12-wide-ls10": ("mask12", "wide", "ls10", ()),
    "mask12-init-ls10": ("mask12", "init", "ls10", ()),
    "mask12-init-ls100": ("mask12", "init", "ls100", ()),
    "pad-wide-ls10": ("pad", "wide", "ls10", ()),
    "pad-init-ls10": ("pad", "init", "ls10", ()),
    "padshift-wide-ls10": ("padshift", "wide", "ls10", ()),
    "padshift-init-ls10": ("padshift", "init", "ls10", ()),
    "padshift-wide-ls100": ("padshift", "wide", "ls100", ()),
    "mask4-wide-ls10-noqkvbias": ("mask4", "wide", "ls10", ("no_qkv_bias",)),
    "padshift-init-ls10-noprojbias": ("padshift", "init", "ls10", ("no_proj_bias",)),
    "mask4-init-ls10-smallx": ("mask4", "init", "ls10", ("small_x",)),          # |x| <= 1e-2: the variance is 3e-5, eps 1e-5
    "flat8-wide-ls10-mean50": ("flat8", "wide", "ls10", ("mean50",)),           # every token's mean is 50
}
MLP_ROWS = (1, 15, 16, 17, 191, 192, 193, 385)   # a lane group, a wave's 16 tokens and a workgroup's 192 rows: one less, whole, one more
MLP_CASES = {f"r{r}-{rec}": (r, rec, ()) for r in MLP_ROWS for rec in ("wide", "init")}
MLP_CASES.update({
    "r193-wide-nob1": (193, "wide", ("no_b1",)),
    "r193-init-nob2": (193, "init", ("no_b2",)),
    "r193-wide-reach": (193, "wide", ("reach",)),                               # LN weight x 2: |hpre| beyond 5 on both sides
    "r193-init-reach": (193, "init", ("reach",)),                               # LN weight x 10
})
SHARP = [n for n, c in ATTN_CASES.items() if c[2] == "ls10" and not c[3]]        # where a dropped cross term of proj must show
SHARP_MLP = [n for n, c in MLP_CASES.items() if not c[2]]


# max |branch32 - branch64| / B per case, the reference in plain fp32 on the CPU against itself in fp64 - measured once, here;
# test_ann_block_bound_cpu.py recomputes each and holds it within a factor 3 (another BLAS or thread count sums in another order).  tol = 8 x this.
R32 = {
    "flat1-wide-ls10": 1.38e-07,
    "flat1-init-ls10": 1.21e-07,
    "flat8-wide-ls10": 1.47e-07,
    "flat8-init-ls100": 1.82e-06,
    "flat12-init-ls10": 1.80e-07,
    "flat12-wide-ls100": 2.16e-06,
    "flat17-wide-ls10": 1.83e-07,
    "flat17-init-ls10": 1.88e-07,
    "mask4-wide-ls10": 1.86e-07,
    "mask4-init-ls10": 2.08e-07,
    "mask4-wide-ls100": 1.40e-06,
    "mask12-wide-ls10": 2.14e-07,
    "mask12-init-ls10": 2.28e-07,
    "mask12-init-ls100": 2.04e-06,
    "pad-wide-ls10": 2.48e-07,
    "pad-init-ls10": 3.46e-07,
    "padshift-wide-ls10": 2.34e-07,
    "padshift-init-ls10": 2.33e-07,
    "padshift-wide-ls100": 1.96e-06,
    "mask4-wide-ls10-noqkvbias": 1.82e-07,
    "padshift-init-ls10-noprojbias": 1.96e-07,
    "mask4-init-ls10-smallx": 1.96e-07,
    "flat8-wide-ls10-mean50": 1.68e-06,
    "r1-wide": 5.70e-08,
    "r1-init": 6.64e-08,
    "r15-wide": 2.24e-07,
    "r15-init": 1.46e-07,
    "r16-wide": 1.34e-07,
    "r16-init": 1.12e-07,
    "r17-wide": 1.38e-07,
    "r17-init": 1.23e-07,
    "r191-wide": 2.66e-07,
    "r191-init": 2.89e-07,
    "r192-wide": 2.55e-07,
    "r192-init": 2.93e-07,
    "r193-wide": 2.77e-07,
    "r193-init": 2.40e-07,
    "r385-wide": 2.95e-07,
    "r385-init": 3.04e-07,
    "r193-wide-nob1": 3.28e-07,
    "r193-init-nob2": 2.00e-07,
    "r193-wide-reach": 3.92e-07,
    "r193-init-reach": 3.93e-07,
}


def tol(name, kind=None):
    """The case's tolerance per unit of B: 8 r32 (the module docstring says what the 8 is made of)."""
    return FACTOR * R32[name]


@dataclass
class AttnCase:
    name: str
    x: torch.Tensor                               # (rows, C)
    row_map: torch.Tensor                         # (B_ * N,) int32
    B_: int
    geom: tuple
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    wqkv: torch.Tensor
    bqkv: torch.Tensor
    wproj: torch.Tensor
    bproj: torch.Tensor
    ls: torch.Tensor                              # raw logit_scale parameter (NH, 1, 1)
    bias: torch.Tensor                            # cpb bias (NH, N, N) fp32: an input of the kernel's table
    mask: torch.Tensor                            # (nW, N, N) or None
    ref: dict = field(default_factory=dict)


@dataclass
class MlpCase:
    name: str
    x: torch.Tensor
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    w1: torch.Tensor
    b1: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    ref: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def attn_case(name):
    gname, recipe, ls, opts = ATTN_CASES[name]
    B, D, H, W, ss = GEOMETRY[gname]
    seed = 21000 + 100 * list(ATTN_CASES).index(name)
    row_map, B_, (Dp, Hp, Wp) = row_map_cpu(B, D, H, W, ss)
    rows = B * D * H * W
    x = rnd((rows, C), seed, -1.5, 1.5)
    if "small_x" in opts:
        x = x * (1e-2 / 1.5)
    if "mean50" in opts:
        x = x + 50.0
    ln_w, ln_b = _norm(seed + 1, recipe)
    sd = {"cpb_mlp.0.weight": _weight((512, 3), seed + 3, recipe), "cpb_mlp.0.bias": _bias(512, seed + 4, recipe),
          "cpb_mlp.2.weight": _weight((NH, 512), seed + 5, recipe)}
    bias = O.ann_cpb_bias(sd, "", NH, WS).contiguous()                           # 16 sigmoid(cpb_mlp(log-spaced offsets)) (:184-189)
    mask = O.compute_mask(Dp, Hp, Wp, WS, ss) if any(ss) else None
    return AttnCase(name, x, row_map, B_, (B, D, H, W, ss), ln_w, ln_b, _weight((3 * C, C), seed + 6, recipe),
                    None if "no_qkv_bias" in opts else _bias(3 * C, seed + 7, recipe), _weight((C, C), seed + 8, recipe),
                    None if "no_proj_bias" in opts else _bias(C, seed + 9, recipe), logit_scale(ls, seed + 10), bias, mask)


@functools.lru_cache(maxsize=None)
def mlp_case(name):
    rows, recipe, opts = MLP_CASES[name]
    seed = 26000 + 100 * list(MLP_CASES).index(name)
    ln_w, ln_b = _norm(seed + 1, recipe)
    if "reach" in opts:
        ln_w = ln_w * (2.0 if recipe == "wide" else 10.0)
    return MlpCase(name, rnd((rows, C), seed, -1.5, 1.5), ln_w, ln_b, _weight((CH, C), seed + 3, recipe),
                   None if "no_b1" in opts else _bias(CH, seed + 4, recipe), _weight((C, CH), seed + 5, recipe),
                   None if "no_b2" in opts else _bias(C, seed + 6, recipe))


# ------------------------------------------------------------------------------------------------ references
def _c(t, dtype):
    return None if t is None else t.to(dtype)


def _scatter(win, row_map, rows):
    """(B_, N, C) per window token -> (rows, C) through the row map; padding tokens dropped.  Every row is some window's token."""
    idx = row_map.long()
    out = win.new_full((rows, win.shape[-1]), float("nan"))
    out[idx[idx >= 0]] = win.reshape(-1, win.shape[-1])[idx >= 0]
    return out


def attn_branch(c: AttnCase, dtype=torch.float64):
    """The attention branch per row of x, in `dtype`, with its intermediates: {"branch" (rows, C), "V" (B_, NH, N, HD), "P" (B_, NH, N, N),
    "O" (B_, N, C), "y" (B_, N, C)}."""
    rows = c.x.shape[0]
    y = F.layer_norm(c.x.to(dtype), (C,), c.ln_w.to(dtype), c.ln_b.to(dtype), EPS)
    idx = c.row_map.long()
    yw = torch.cat([y, y.new_zeros(1, C)])[torch.where(idx >= 0, idx, torch.tensor(rows))].view(c.B_, N, C)   # padding: zeros BEHIND the norm
    qkv = yw @ c.wqkv.to(dtype).T
    if c.bqkv is not None:
        qkv = qkv + c.bqkv.to(dtype)
    ls = torch.clamp(c.ls.to(dtype), max=LN100).exp()
    o, p = O.ann_attention_core(qkv, ls, c.bias.to(dtype), _c(c.mask, dtype), NH)
    br = o @ c.wproj.to(dtype).T
    if c.bproj is not None:
        br = br + c.bproj.to(dtype)
    v = qkv.reshape(c.B_, N, 3, NH, HD)[:, :, 2].permute(0, 2, 1, 3)
    return {"branch": _scatter(br, c.row_map, rows), "V": v, "P": p, "O": o, "y": yw}


def mlp_branch(c: MlpCase, dtype=torch.float64):
    """The MLP branch in `dtype`: {"branch", "hpre" (before GELU), "H", "y"}."""
    y = F.layer_norm(c.x.to(dtype), (C,), c.ln_w.to(dtype), c.ln_b.to(dtype), EPS)
    hpre = y @ c.w1.to(dtype).T
    if c.b1 is not None:
        hpre = hpre + c.b1.to(dtype)
    h = F.gelu(hpre)
    br = h @ c.w2.to(dtype).T
    if c.b2 is not None:
        br = br + c.b2.to(dtype)
    return {"branch": br, "hpre": hpre, "H": h, "y": y}


def attn_ref(name):
    """fp64 reference and the magnitude sum B of one attention case (computed once, shared, never modified)."""
    c = attn_case(name)
    if not c.ref:
        r = attn_branch(c)
        rows = c.x.shape[0]
        wp = c.wproj.double().abs()
        oabs = (r["P"] @ r["V"].abs()).transpose(1, 2).reshape(c.B_, N, C)
        mag = oabs @ wp.T + (0 if c.bproj is None else c.bproj.double().abs())
        c.ref.update(branch=r["branch"], B=_scatter(mag, c.row_map, rows))
        assert not torch.isnan(c.ref["branch"]).any(), "a row of x that no window maps"
    return c.ref


def mlp_ref(name):
    c = mlp_case(name)
    if not c.ref:
        r = mlp_branch(c)
        w2 = c.w2.double().abs()
        mag = r["H"].abs() @ w2.T + (0 if c.b2 is None else c.b2.double().abs())
        c.ref.update(branch=r["branch"], B=mag, gelu=GELU_ABS * (r["hpre"].abs() @ w2.T), hpre=r["hpre"])
    return c.ref


def r32(name, kind):
    """max over elements |branch32 - branch64| / B: how far the reference itself is from fp64 when evaluated in plain fp32."""
    c, ref = (attn_case(name), attn_ref(name)) if kind == "attn" else (mlp_case(name), mlp_ref(name))
    b32 = (attn_branch if kind == "attn" else mlp_branch)(c, torch.float32)["branch"].double()
    return ((b32 - ref["branch"]).abs() / ref["B"]).max().item()


def worst_ratio(out, name, kind, tol):
    """max over elements |(out - x) - branch64| / allowance for a result `out` (rows, C) fp32 of x + branch."""
    c, ref = (attn_case(name), attn_ref(name)) if kind == "attn" else (mlp_case(name), mlp_ref(name))
    x64 = c.x.double()
    allow = tol * ref["B"] + 2.0 ** -23 * (x64 + ref["branch"]).abs()
    if kind == "mlp":
        allow = allow + ref["gelu"]
    return (((out.double() - x64) - ref["branch"]).abs() / allow).max().item()


# ------------------------------------------------------------------------------------------------ emulation of the kernels' numerics
_FTZ = [False]                                   # set by the emulations for the length of one call


def split(x):
    """fp32 -> (hi, lo) as fp32 values of fp16 numbers: hi = fp16(x), lo = fp16(x - hi) (csrc/f16_split.h: split2).  Under ftz the
    operand is what a matrix pipe that flushes fp16 subnormals would see: every half below 2^-14 is zero."""
    hi = x.half().float()
    lo = (x - hi).half().float()
    if _FTZ[0]:
        hi, lo = torch.where(hi.abs() < 2.0 ** -14, 0.0, hi), torch.where(lo.abs() < 2.0 ** -14, 0.0, lo)
    return hi, lo


def prod3(a, b, drop=None):
    """a b^T as mma3 computes it: a_hi b_lo + a_lo b_hi + a_hi b_hi (the smallest first), fp32 sums; `drop` in {"hi_lo", "lo_hi",
    "hi_hi"} omits that term - (a, b) are mma3's operands in the kernel's call, e.g. proj: a = Wp, b = O; "lo_hi" is a_lo b_hi."""
    ah, al = split(a)
    bh, bl = split(b)
    t = [None if drop == "hi_lo" else ah @ bl.transpose(-1, -2), None if drop == "lo_hi" else al @ bh.transpose(-1, -2),
         None if drop == "hi_hi" else ah @ bh.transpose(-1, -2)]
    t = [u for u in t if u is not None]
    acc = t[0]
    for u in t[1:]:
        acc = acc + u
    return acc


def _ln32(x, w, b):
    """LayerNorm as the kernels do it: mean, biased variance of the centred values, 1 / sqrt, all fp32."""
    mean = x.sum(-1, keepdim=True) * (1.0 / C)
    t = x - mean
    rstd = 1.0 / torch.sqrt((t * t).sum(-1, keepdim=True) * (1.0 / C) + torch.tensor(EPS))
    return t * rstd * w + b


def _d(drop, product):
    return drop[1] if drop is not None and drop[0] == product else None


def _attn_emulate(c: AttnCase, drop):
    """x + branch in the numerics csrc/ann_block.hip documents (fp32 LayerNorm; every product on fp16 hi / lo operands, three terms, fp32
    sums: qkv, K Q^T, V^T P^T, proj; the softmax in the log2 domain on top of the (bias + mask) * log2 e table; unnormalised
    probabilities split, O divided by the row sum and split).  drop = (product, term), product in {"qkv", "qk", "pv", "proj"}."""
    rows = c.x.shape[0]
    y = _ln32(c.x, c.ln_w, c.ln_b)
    idx = c.row_map.long()
    yw = torch.cat([y, y.new_zeros(1, C)])[torch.where(idx >= 0, idx, torch.tensor(rows))].view(c.B_, N, C)
    # q, k: the weights are mma3's `a`; v: the tokens are.  (B_, N, 3C)
    qk = prod3(c.wqkv[:2 * C], yw, _d(drop, "qkv")).transpose(-1, -2)
    v = prod3(yw, c.wqkv[2 * C:], _d(drop, "qkv"))
    if c.bqkv is not None:
        qk, v = qk + c.bqkv[:2 * C], v + c.bqkv[2 * C:]
    heads = lambda t: t.reshape(c.B_, N, NH, HD).permute(0, 2, 1, 3)              # (B_, NH, N, HD)
    q, k, v = heads(qk[..., :C]), heads(qk[..., C:]), heads(v)
    scale2 = (torch.clamp(c.ls, max=LN100).exp().reshape(-1) * LOG2E).view(1, NH, 1, 1)        # hip.ann_attn_block_table
    table = ((c.bias[None] if c.mask is None else c.bias[None] + c.mask[:, None]) * LOG2E)     # (nW, NH, N, N)
    q = q * (scale2 / torch.sqrt((q * q).sum(-1, keepdim=True)).clamp_min(1e-12))
    k = k * (1.0 / torch.sqrt((k * k).sum(-1, keepdim=True)).clamp_min(1e-12))
    s = prod3(k, q, _d(drop, "qk")).transpose(-1, -2)                              # (B_, NH, query, key): a = K, b = Q
    nW = table.shape[0]
    s = (s.view(c.B_ // nW, nW, NH, N, N) + table[None]).view(c.B_, NH, N, N)
    e = torch.exp2(s - s.max(-1, keepdim=True).values)
    inv = 1.0 / e.sum(-1, keepdim=True)
    o = prod3(v.transpose(-1, -2), e, _d(drop, "pv")).transpose(-1, -2) * inv      # a = V^T, b = P
    o = o.permute(0, 2, 1, 3).reshape(c.B_, N, C)
    br = prod3(c.wproj, o, _d(drop, "proj")).transpose(-1, -2)                     # a = Wp, b = O
    if c.bproj is not None:
        br = br + c.bproj
    return _scatter(br, c.row_map, rows) + c.x


def attn_emulate(c, drop=None, ftz=False):
    """_attn_emulate; ftz: on a matrix pipe that flushes fp16 subnormal inputs to zero."""
    _FTZ[0] = ftz
    try:
        return _attn_emulate(c, drop)
    finally:
        _FTZ[0] = False


def gelu_poly(x):
    """gelu_erfc_poly of csrc/ann_mlp_block.hip (Abramowitz & Stegun 7.1.26), fp32."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    u = x.abs() * f(0.70710678118654752440)
    t = 1.0 / (f(0.3275911) * u + 1.0)
    p = t * f(0.5 * 1.061405429) + f(0.5 * -1.453152027)
    p = t * p + f(0.5 * 1.421413741)
    p = t * p + f(0.5 * -0.284496736)
    p = t * p + f(0.5 * 0.254829592)
    q = p * t * torch.exp2(u * u * f(-1.4426950408889634))
    xq = x * q
    return torch.where(x < 0, xq, x - xq)


def _mlp_emulate(c: MlpCase, drop):
    """x + branch in the numerics csrc/ann_mlp_block.hip documents.  drop = (product, term), product in {"fc1", "fc2"}."""
    y = _ln32(c.x, c.ln_w, c.ln_b)
    hpre = prod3(c.w1, y, _d(drop, "fc1")).transpose(-1, -2)                       # a = W1, b = LN(x)
    if c.b1 is not None:
        hpre = hpre + c.b1
    br = prod3(c.w2, gelu_poly(hpre), _d(drop, "fc2")).transpose(-1, -2)           # a = W2, b = H
    if c.b2 is not None:
        br = br + c.b2
    return br + c.x


def mlp_emulate(c, drop=None, ftz=False):
    """_mlp_emulate; ftz as in attn_emulate."""
    _FTZ[0] = ftz
    try:
        return _mlp_emulate(c, drop)
    finally:
        _FTZ[0] = False
