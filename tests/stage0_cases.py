"""Inputs, CPU references and checks of tests/test_stage0_parity_gpu.py (plain CPU code, no GPU call in here): the patch embedding's head
convolution, the flow-prediction head, the one-launch first half of the QK attention, the one-launch MS MLP and the token gate.

Every builder is cached: the routes of the test file share one reference per case, and nothing mutates what a builder returned.

Neurons.  `neuron(name, v_th, ...)` makes one of the seven named settings; the compile-time class the library sorts it into (spike_mm.h
neuron_class) is CLASS[name]:
  lif       LIF, tau 2, soft reset                                   class 0
  plif      LIF, tau = k = 0.3775406777858734, soft reset            class 0, the multiplicative charge of ParametricLIFNode
  lif_hard  LIF, tau 2, v_reset 0                                    class 2
  lif_vr    LIF, tau 2, v_reset 0.05                                 class 2, the initial membrane and the charge use v_reset
  lif_tau3  LIF, tau 3, soft reset                                   class 2 through the division
  if        IF, soft reset                                           class 2
  psn       PSN, W = random + 0.5 I, b = -0.1 (or as the case says)  class 1
Where a kernel takes several neurons they get DIFFERENT settings of one class (other thresholds, lif beside plif, other PSN matrices, a
mix of the class-2 settings), so that a kernel which reads one neuron's field for another cannot pass.

Head convolution, two kinds of operands:
  exact   integer event counts in [-3, 3] (about 60 % zeros), weights k / 8 with |k| <= 4, alpha in {0.5, 1, 2}, beta k / 16 with
          |k| <= 8, PSN W = k / 8 + 0.5 I and b = -0.125: every partial sum of the convolution is a multiple of 1/8 below 2^6, BatchNorm
          a multiple of 1/16 below 2^8, a PSN membrane a multiple of 2^-7 below 2^12 - exact in fp32 in ANY summation order (the fmaf
          chain of head_conv_sn_kernel, v_mfma_f32_32x32x2_f32, float64).  The neuron arithmetic is the separately rounded sequence
          oracle/csrc/neuron_ref.c restates, so the spikes must EQUAL neuron_ref of the float64 convolution cast to fp32.
  random  the recipe of test_hip_kernels.py::test_head_conv_bn_neuron: real values in (-1, 3) with |x| < 0.8 zeroed, real alpha / beta.
          Checked with O.delta_consistent, delta = 16 * 2^-23 * max(rms, v_th) (tests/replay.py's rule); the premise - that an fp32
          evaluation in the kernel's documented (ky, kx, cin) order passes the same check - is `head_emulated`.
"""
import functools

import numpy as np
import torch

import spike_conv_cases as SC
import spike_gemm_cases as G
from oracle import neuron_ref as R
from oracle import sdformer_oracle as O
from sdformerflow_amd.synthetic import synth_uniform as rnd

PLIF_K = 0.3775406777858734
SETTINGS = {"lif": ("lif", 2.0, None), "plif": ("lif", PLIF_K, None), "lif_hard": ("lif", 2.0, 0.0), "lif_vr": ("lif", 2.0, 0.05),
            "lif_tau3": ("lif", 3.0, None), "if": ("if", 2.0, None), "psn": ("psn", 2.0, None)}       # name -> (kind, tau, v_reset)
CLASS = {"lif": 0, "plif": 0, "psn": 1, "lif_hard": 2, "lif_vr": 2, "lif_tau3": 2, "if": 2}
NAMES = tuple(SETTINGS)
CLASS2 = ("lif_hard", "lif_vr", "lif_tau3", "if")
DELTA_ULPS = G.DELTA_ULPS
AMBIGUOUS_CAP, FLIP_CAP, RANGE_TOL = 1e-4, 2e-4, 1e-5       # the project's bounds: tests/replay.py, test_ms_mlp_fused_gpu.py


class Neuron:
    """One neuron setting on the CPU: what hip.NeuronParams takes, the reference neuron over dim 0 and the delta check."""

    def __init__(self, name, v_th, psn_w=None, psn_b=None):
        self.name, self.v_th, self.psn_w, self.psn_b = name, float(v_th), psn_w, psn_b
        self.kind, self.tau, self.v_reset = SETTINGS[name]
        self.cls = CLASS[name]

    def ref(self, x):
        """spikes (same shape, fp32) of x (T, ...) fp32"""
        return R.neuron_ref(x, self.kind, self.tau, self.v_th, self.v_reset, psn_w=self.psn_w, psn_b=self.psn_b)

    def report(self, x, got):
        """O.delta_consistent of `got` for the pre-activation x (T, ...) fp32 under the project's delta rule; + the delta used"""
        x = x.contiguous()
        delta = DELTA_ULPS * 2.0 ** -23 * max(float(x.double().pow(2).mean().sqrt()), self.v_th)
        rep = O.delta_consistent(x, got.float().contiguous(), O.NeuronCfg(self.kind, self.v_th, self.v_reset, self.tau, x.shape[0]),
                                 {"w.weight": self.psn_w, "w.bias": self.psn_b}, "w.", delta)
        rep["delta"] = delta
        return rep

    def same_settings(self, o):
        return (self.kind, self.tau, self.v_th, self.v_reset) == (o.kind, o.tau, o.v_th, o.v_reset) and self.psn_w is o.psn_w


@functools.lru_cache(maxsize=None)
def neuron(name, v_th, T=0, seed=0, exact=False, centre=None):
    """The named setting at threshold v_th.  psn: its own T x T matrix per seed; `exact`: on the grid of the exact head cases; `centre`:
    b[t] = -centre * sum_k W[t][k], which puts the membrane of inputs around `centre` around zero (the token gates, whose inputs are
    head sums far from zero)."""
    if name != "psn":
        return Neuron(name, v_th)
    if exact:
        g = np.random.Generator(np.random.PCG64(7100 + 13 * T + seed))
        W = torch.from_numpy((g.integers(-4, 5, (T, T)) / 8.0).astype(np.float32)) + 0.5 * torch.eye(T)
        return Neuron(name, v_th, W.contiguous(), torch.full((T,), -0.125))
    W = (rnd((T, T), 7200 + 13 * T + seed, -0.5, 0.5) + 0.5 * torch.eye(T)).contiguous()
    b = torch.full((T,), -0.1) if centre is None else (-centre * W.sum(1)).contiguous()
    return Neuron(name, v_th, W, b)


def check_rate(s, lo=0.03, hi=0.97):
    r = float(s.float().mean())
    assert lo < r < hi, r
    return r


def check_report(rep, flips=False):
    """0 unexplained decisions; at most 1e-4 of them ambiguous (2e-4 differ from the reference's where the issue bounds the flips)"""
    assert rep["unexplained"] == 0, rep
    if flips:
        assert rep["flips"] <= FLIP_CAP * rep["n"], rep
    else:
        assert rep["ambiguous"] <= AMBIGUOUS_CAP * rep["n"], rep
    return rep


# ---------------------------------------------------------------------------------------------------- 1. head convolution
HEAD_T = (5, 10, 20)
HEAD_PAIRS = ((2, 48), (2, 32), (2, 64), (4, 48))
HEAD_PSN_MFMA = {(T, p) for T in (5, 10) for p in ((2, 48), (2, 32))}      # head_conv_mfma_psn_kernel's instantiations
# thresholds of the exact / the random head cases (the exact pre-activations are a few units wide, the random ones about one)
HEAD_VTH = {"exact": {"lif": 0.25, "plif": 0.1875, "lif_hard": 0.3125, "lif_vr": 0.375, "lif_tau3": 0.21875, "if": 0.75, "psn": 0.0},
            "random": {"lif": 0.1, "plif": 0.08, "lif_hard": 0.12, "lif_vr": 0.15, "lif_tau3": 0.09, "if": 0.3, "psn": 0.0}}


def head_neuron(name, T, exact):
    return neuron(name, HEAD_VTH["exact" if exact else "random"][name], T if name == "psn" else 0, 0, exact and name == "psn")


@functools.lru_cache(maxsize=None)
def head_inputs(T, Cin, Cout, B, H, W, exact, bn=True):
    """x (B T, H, W, Cin) fp32 NHWC with image b T + t, w (Cout, Cin, 3, 3), alpha / beta (Cout,) or None, pre64 = BN(conv) in float64 as
    (T, B, H, W, Cout), pre = its fp32 cast."""
    seed = 7300 + 101 * T + 7 * Cin + Cout + 3 * B + 5 * H + W + (0 if bn else 50)
    if exact:
        g = np.random.Generator(np.random.PCG64(seed))
        mag = g.integers(1, 4, (B * T, H, W, Cin)) * (g.integers(0, 2, (B * T, H, W, Cin)) * 2 - 1)
        x = torch.from_numpy((mag * (g.random((B * T, H, W, Cin)) < 0.4)).astype(np.float32))
        w = torch.from_numpy((g.integers(-4, 5, (Cout, Cin, 3, 3)) / 8.0).astype(np.float32))
        alpha = torch.from_numpy(g.choice(np.array([0.5, 1.0, 2.0], np.float32), Cout))
        beta = torch.from_numpy((g.integers(-8, 9, Cout) / 16.0).astype(np.float32))
    else:
        x = rnd((B * T, H, W, Cin), seed, -1.0, 3.0)
        x[x.abs() < 0.8] = 0.0
        w = rnd((Cout, Cin, 3, 3), seed + 1, -0.5, 0.5)
        alpha, beta = rnd((Cout,), seed + 2, 0.5, 1.5), rnd((Cout,), seed + 3, -0.2, 0.2)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    if bn:
        y = y * alpha.double() + beta.double()
    else:
        alpha = beta = None
    pre64 = y.reshape(B, T, H, W, Cout).permute(1, 0, 2, 3, 4).contiguous()
    return {"T": T, "Cin": Cin, "Cout": Cout, "B": B, "H": H, "W": W, "x": x, "w": w, "alpha": alpha, "beta": beta, "pre64": pre64,
            "pre": pre64.float().contiguous()}


@functools.lru_cache(maxsize=None)
def head_spikes(T, Cin, Cout, B, H, W, exact, bn, name):
    """(the reference's spikes as the kernel lays them out: (B, T, H, W, Cout) u8, the neuron)"""
    c, n = head_inputs(T, Cin, Cout, B, H, W, exact, bn), head_neuron(name, T, exact)
    return n.ref(c["pre"]).permute(1, 0, 2, 3, 4).contiguous().to(torch.uint8), n


def head_voxel(c, spare):
    """The packed input of a head case as the event voxel (B, bins, 2, H, W) the kernel reads in place: channel ci of step t is polarity
    ci % 2 of bin (ci // 2) T + t; `spare` more bins behind them, all NaN (the kernel has no business there)."""
    B, T, H, W, Cin = c["B"], c["T"], c["H"], c["W"], c["Cin"]
    bins = (Cin // 2) * T + spare
    vox = torch.full((B, bins, 2, H, W), float("nan"))
    xv = c["x"].view(B, T, H, W, Cin)
    for ci in range(Cin):
        vox[:, (ci // 2) * T:(ci // 2 + 1) * T, ci % 2] = xv[..., ci]
    return vox.contiguous(), bins


def head_emulated(c):
    """The head's pre-activation evaluated in fp32 the way the kernels document it: one fmaf chain per output over (ky, kx, cin) from 0,
    taps outside the image contributing x = 0, then BatchNorm as fmaf(acc, alpha, beta).  (fmaf through float64: the product of two fp32
    values is exact there.)  -> (T, B, H, W, Cout) fp32."""
    B, T, H, W, Cin, Cout = c["B"], c["T"], c["H"], c["W"], c["Cin"], c["Cout"]
    xp = torch.nn.functional.pad(c["x"].permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1).double()
    acc = torch.zeros((B * T, H, W, Cout))
    for ky in range(3):
        for kx in range(3):
            for ci in range(Cin):
                acc = (xp[:, ky:ky + H, kx:kx + W, ci, None] * c["w"][:, ci, ky, kx].double() + acc.double()).float()
    if c["alpha"] is not None:
        acc = (acc.double() * c["alpha"].double() + c["beta"].double()).float()
    return acc.view(B, T, H, W, Cout).permute(1, 0, 2, 3, 4).contiguous()


def head_route(c, name, mfma=True):
    """The one launch of hip.head_conv_sn for a case, as routes_common.logged prints it (csrc/head_tail.hip launch_head and
    sdf_head_conv_sn_fwd: the matrix-pipe kernels want W % 32 == 0 and, for PSN, an instantiation; they run min(ceil(tiles / 4), 768)
    workgroups over B H W / 32 tiles; the 16-pixel kernel one workgroup per 16 pixels)."""
    T, Cin, Cout, B, H, W = (c[k] for k in ("T", "Cin", "Cout", "B", "H", "W"))
    psn = name == "psn"
    if mfma and W % 32 == 0 and (not psn or (T, (Cin, Cout)) in HEAD_PSN_MFMA):
        wgs = min((B * H * (W // 32) + 3) // 4, 768)
        if psn:
            return [f"{wgs} 256 0 head_conv_mfma_psn_kernel<{T}, {Cin}, {Cout}>"]
        return [f"{wgs} 256 0 head_conv_mfma_kernel<{T}, {Cin}, {Cout}, {'true' if CLASS[name] == 0 else 'false'}>"]
    return [f"{B * H * (W // 16)} 256 0 head_conv_sn_kernel<{T}, {Cout // 16}, {Cin}>"]


# ---------------------------------------------------------------------------------------------------- 2. prediction head
PRED_D, PRED_CIN = (5, 10, 20), (96, 192, 384)
PRED_SHAPES = ((1, 3, 4, 1, 1), (2, 5, 7, 2, 2), (1, 3, 4, 16, 16), (2, 5, 7, 2, 4))          # (B, h, w, sy, sx)
PRED_VTH = {"lif": 0.1, "plif": 0.12, "lif_hard": 0.1, "lif_vr": 0.12, "lif_tau3": 0.08, "if": 0.4, "psn": 0.0}


def pred_neurons(D, Cin, cls, same_next=False):
    """(sn_pred, sn_next) of one instantiation: two settings of the class, rotated over (D, Cin) so that every class-2 setting stands at
    every D (three widths x two neurons) and plif on both sides of class 0; sn_next's threshold is 1.5 x the table's."""
    i = PRED_D.index(D) + PRED_CIN.index(Cin)
    names = {0: (("lif", "plif"), ("plif", "lif"))[i % 2], 1: ("psn", "psn"), 2: (CLASS2[i % 4], CLASS2[(i + 1) % 4])}[cls]
    sn = neuron(names[0], PRED_VTH[names[0]], D, 1)
    return sn, sn if same_next else neuron(names[1], 1.5 * PRED_VTH[names[1]], D, 2)


@functools.lru_cache(maxsize=None)
def pred_case(D, Cin, cls, shape, bias=True, same_next=False):
    B, h, w, sy, sx = PRED_SHAPES[shape]
    seed = 7400 + 11 * D + Cin + 3 * shape
    z = rnd((B, D, h, w, Cin), seed, -0.5, 1.0)
    sn, sn_next = pred_neurons(D, Cin, cls, same_next)
    zt = z.permute(1, 0, 2, 3, 4).contiguous()
    c = {"B": B, "D": D, "h": h, "w": w, "Cin": Cin, "H": h * sy, "W": w * sx, "z": z, "wgt": rnd((2, Cin), seed + 1, -0.3, 0.3),
         "bias": rnd((2,), seed + 2, -0.2, 0.2) if bias else None, "sn": sn, "sn_next": sn_next,
         "sp": sn.ref(zt).permute(1, 0, 2, 3, 4).contiguous(), "next_z": sn_next.ref(zt).permute(1, 0, 2, 3, 4).contiguous()}
    lpp = Cin // 12
    c["route"] = [f"{-(-B * h * w // (4 * (64 // lpp)))} 256 0 pred_head_kernel<{D}, {lpp}, {cls}>"]
    return c


def pred_reference(c, sp):
    """(pred (B, D, h, w, 2), flow (B, 2, H, W)) in float64 on the spikes `sp` (B, D, h, w, Cin)"""
    p64 = sp.double() @ c["wgt"].double().t() + (c["bias"].double() if c["bias"] is not None else 0.0)
    f64 = torch.nn.functional.interpolate(p64.sum(1).permute(0, 3, 1, 2), scale_factor=(c["H"] // c["h"], c["W"] // c["w"]))
    return p64, f64


def pred_next_of_pred(c, pred2):
    """SN_next over D of the two prediction channels (B, D, h, w, 2) fp32 -> the same shape"""
    return c["sn_next"].ref(pred2.permute(1, 0, 2, 3, 4).contiguous()).permute(1, 0, 2, 3, 4)


# ---------------------------------------------------------------------------------------------------- 3. one-launch QK front
QK_GEOM = {"w5": (1, 2, 5, 5, (2, 5, 5), (0, 0, 0)),            # one window of 25 tokens
           "w8": (1, 2, 8, 8, (2, 8, 8), (0, 0, 0)),            # 64 tokens: two token blocks of the kernel
           "w9": (1, 4, 11, 13, (2, 9, 9), (1, 4, 4))}          # 81 tokens, shifted, the map padded to 4 x 18 x 18: 8 windows
QK_VTH = {"lif": 0.1, "plif": 0.12, "lif_hard": 0.1, "lif_vr": 0.12, "lif_tau3": 0.08, "if": 0.3, "psn": 0.0}


def slice_map(B, D, H, W, ws, ss):
    """sdf_window_slice_map restated (csrc/qk_attn.hip slice_map_kernel): int32 (B_ Wd Wh Ww,), -1 = padding; and B_"""
    Wd, Wh, Ww = ws
    N1 = Wh * Ww
    Dp, Hp, Wp = -(-D // Wd) * Wd, -(-H // Wh) * Wh, -(-W // Ww) * Ww
    nD, nHb, nWb = Dp // Wd, Hp // Wh, Wp // Ww
    B_ = B * nD * nHb * nWb
    i = np.arange(B_ * Wd * N1, dtype=np.int64)
    tok, j = i % N1, i // N1
    wd, win = j % Wd, j // Wd
    wb, hb, db, b = win % nWb, (win // nWb) % nHb, (win // (nWb * nHb)) % nD, win // (nWb * nHb * nD)
    d, h, w = (db * Wd + wd + ss[0]) % Dp, (hb * Wh + tok // Ww + ss[1]) % Hp, (wb * Ww + tok % Ww + ss[2]) % Wp
    m = np.where((d < D) & (h < H) & (w < W), ((b * D + d) * H + h) * W + w, -1)
    return torch.from_numpy(m.astype(np.int32)), B_


def qk_neurons(cls, form, Cc):
    """(sn_proj, sn_q, sn_k, sn2_q) of one class, all different - except that the stacked projection is one product with ONE neuron
    (include/sdformerflow_hip.h: "valid when the q and k neurons are parameter-free and equal"), so there sn_k is sn_q.  sn2_q sees
    head sums of 32 spikes at rate about 0.45: its threshold sits where the gate fires about half the time."""
    if cls == 0:
        names, gate_th = ("plif", "lif", "plif", "lif"), 7.0
    elif cls == 1:
        names, gate_th = ("psn",) * 4, 0.0
    else:
        names, gate_th = ("lif_vr", "lif_tau3", "if", "lif_hard"), 7.0
    ns = [neuron(nm, QK_VTH[nm] * (1.0 + 0.25 * i), 2, 10 + i) for i, nm in enumerate(names[:3])]
    ns.append(neuron(names[3], gate_th, 2, 13, centre=14.0 if cls == 1 else None))
    if form == "stacked":
        ns[2] = ns[1]
    return tuple(ns)


def held2(W):
    """the float64 value of W as two fp16 planes hold it (spike_conv_cases.held_weights; the GPU test compares with the device's planes)"""
    return SC.held_weights(W, 2)


@functools.lru_cache(maxsize=None)
def qk_case(Cc, geom, form, cls):
    """x (B, D, H, W, C); the q / k / output projections with their BatchNorms, the positional table pe (Tq N1, C); the reference's slice
    spikes, the float64 pre-activations of q and k cast to fp32 as (Tq, B_ N1, C), and the reference's own q / k / gate."""
    B, D, H, W, window, shift = QK_GEOM[geom]
    Tq, N1, nH = window[0], window[1] * window[2], Cc // 32
    seed = 7500 + Cc + 7 * N1 + 3 * cls + (1 if form == "stacked" else 0)
    x = rnd((B, D, H, W, Cc), seed, -0.5, 1.0)
    lin = {k: {"W": rnd((Cc, Cc), seed + 10 * i + 1, -0.2, 0.2), "alpha": rnd((Cc,), seed + 10 * i + 2, 0.5, 1.5),
               "beta": rnd((Cc,), seed + 10 * i + 3, -0.2, 0.2)} for i, k in enumerate(("q", "k", "p"))}
    lin["p"]["bias"] = rnd((Cc,), seed + 40, -0.1, 0.1)
    pe = rnd((Tq * N1, Cc), seed + 41, -0.3, 0.3)
    m, B_ = slice_map(B, D, H, W, window, shift)
    rows = B_ * N1
    sn_proj, sn_q, sn_k, sn2_q = qk_neurons(cls, form, Cc)
    xg = torch.zeros((Tq * rows, Cc))
    xg[m >= 0] = x.reshape(-1, Cc)[m[m >= 0].long()]
    sproj = sn_proj.ref(xg.view(Tq, rows, Cc).contiguous())
    if form == "stacked":
        Wh = held2(torch.cat([lin["q"]["W"], lin["k"]["W"]], 0))
        held = {"q": Wh[:Cc], "k": Wh[Cc:]}
    else:
        held = {"q": held2(lin["q"]["W"]), "k": held2(lin["k"]["W"])}
    c = {"Cc": Cc, "nH": nH, "Tq": Tq, "N1": N1, "B_": B_, "rows": rows, "geom": QK_GEOM[geom], "form": form, "cls": cls, "x": x, "lin": lin,
         "pe": pe, "map": m, "held": held, "sproj": sproj, "sn": (sn_proj, sn_q, sn_k, sn2_q)}
    c["pre_q"], c["pre_k"] = qk_pre(c, sproj)
    c["q"], c["k"] = sn_q.ref(c["pre_q"]), sn_k.ref(c["pre_k"])
    c["gate"] = qk_gate_of(c, c["q"])
    c["route"] = f"{B_ * nH} 256 0 qk_front_kernel<{cls}, %s>"
    return c


def qk_pre(c, sproj):
    """BN(SN_proj(x) W^T) (+ pe on k) in float64 on the slice spikes `sproj` (Tq, rows, C), cast to fp32"""
    Tq, N1, rows, Cc = c["Tq"], c["N1"], c["rows"], c["Cc"]
    out = []
    for k in ("q", "k"):
        y = (sproj.double() @ c["held"][k].t()) * c["lin"][k]["alpha"].double() + c["lin"][k]["beta"].double()
        if k == "k":
            y = y + c["pe"].double().view(Tq, 1, N1, Cc).expand(Tq, c["B_"], N1, Cc).reshape(Tq, rows, Cc)
        out.append(y.float().contiguous())
    return out


def qk_gate_of(c, q):
    """SN2_q over the Tq steps of the head sums (exact integers) of q (Tq, rows, C) -> (Tq, rows, nH)"""
    return c["sn"][3].ref(q.float().view(c["Tq"], c["rows"], c["nH"], 32).sum(3).contiguous())


def qk_tape(c, qk):
    """(q, k) as (Tq, rows, C) u8 from the tape's q | k region: one (M, 2C) matrix for the stacked form, q's then k's (M, C) otherwise"""
    Tq, rows, Cc = c["Tq"], c["rows"], c["Cc"]
    M = Tq * rows
    if c["form"] == "stacked":
        both = qk[:M * 2 * Cc].view(Tq, rows, 2 * Cc)
        return both[..., :Cc].contiguous(), both[..., Cc:].contiguous()
    return qk[:M * Cc].view(Tq, rows, Cc), qk[M * Cc:2 * M * Cc].view(Tq, rows, Cc)


def qk_check(c, q, k, e):
    """The oracle, step by step, on what the kernel left: q | k delta-consistent with the float64 pre-activation on the REFERENCE's slice
    spikes (SN_proj is elementwise on x: the kernel's are the reference's bit for bit, or q | k fail here); E = k AND SN2_q(head sums of
    the kernel's OWN q), bit for bit.  -> the two reports."""
    _, sn_q, sn_k, _ = c["sn"]
    rq, rk = check_report(sn_q.report(c["pre_q"], q), flips=True), check_report(sn_k.report(c["pre_k"], k), flips=True)
    gate = qk_gate_of(c, q)
    want = (k.view(c["Tq"], c["rows"], c["nH"], 32).float() * gate[..., None]).view(c["Tq"], c["rows"], c["Cc"]).to(torch.uint8)
    assert torch.equal(e, want), f"E differs from k AND SN2_q(head sums of q) in {int((e != want).sum())} of {e.numel()} bytes"
    return rq, rk


# ---------------------------------------------------------------------------------------------------- 4. one-launch MS MLP
MLP_VTH = {"lif": 0.1, "plif": 0.12, "lif_hard": 0.1, "lif_vr": 0.12, "lif_tau3": 0.08, "if": 0.4, "psn": 0.0}
MLP_SHAPES = ((1, 3, 5), (2, 5, 7))                       # (B, H, W): 15 positions - below every work item's share - and 70


def mlp_neurons(cls, D, C):
    """(sn1, sn2): two settings of the class; the class-2 pair rotates over (D, C)"""
    i = (5, 10, 20).index(D) * 2 + (96, 192).index(C)
    names = {0: ("lif", "plif") if i % 2 == 0 else ("plif", "lif"), 1: ("psn", "psn"), 2: (CLASS2[i % 4], CLASS2[(i + 2) % 4])}[cls]
    return neuron(names[0], MLP_VTH[names[0]], D, 20), neuron(names[1], 1.25 * MLP_VTH[names[1]], D, 21)


def mlp_geometry(ns, D, C):
    """(positions per work item, teams, threads) of ms_mlp_fused_kernel<ns, D, C / 16, CG, NB1, RG, TEAMS, ..> (csrc/ms_mlp_fused.hip
    MlpGeo and launch_t) and the template arguments between T and the neuron class"""
    cg, nb1 = (3, 2) if C == 96 else (4, 1)
    rg = (4 if ns == 3 else 2) if C == 96 else 1
    teams = 2 if C == 96 and ns != 3 else 1
    return 4 * (20 // D) * rg, teams, teams * 64 * rg * cg, (C // 16, cg, nb1, rg, teams)


@functools.lru_cache(maxsize=None)
def mlp_case(D, C, cls, ns=2, shape=0):
    B, H, W = MLP_SHAPES[shape]
    Ch = 4 * C
    seed = 7600 + 11 * D + C + 3 * shape
    sn1, sn2 = mlp_neurons(cls, D, C)
    x = rnd((B, D, H, W, C), seed, -0.5, 1.0)
    fc1 = {"W": rnd((Ch, C), seed + 1, -0.3, 0.3), "alpha": rnd((Ch,), seed + 3, 0.5, 1.5), "beta": rnd((Ch,), seed + 4, -0.2, 0.2)}
    fc2 = {"W": rnd((C, Ch), seed + 2, -0.1, 0.1), "alpha": rnd((C,), seed + 5, 0.5, 1.5), "beta": rnd((C,), seed + 6, -0.2, 0.2)}
    for f in (fc1, fc2):
        f["held"] = SC.held_weights(f["W"], ns)
    ntok = B * D * H * W
    s1 = sn1.ref(x.permute(1, 0, 2, 3, 4).contiguous()).permute(1, 0, 2, 3, 4).reshape(ntok, C).to(torch.uint8)
    ppi, teams, threads, geo = mlp_geometry(ns, D, C)
    wgs = -(-(-(-B * H * W // ppi)) // teams)
    targs = ", ".join(str(a) for a in (ns, D) + geo + (cls,))
    return {"B": B, "D": D, "H": H, "W": W, "C": C, "Ch": Ch, "ns": ns, "ntok": ntok, "x": x, "fc1": fc1, "fc2": fc2, "sn1": sn1, "sn2": sn2,
            "s1": s1, "route": f"{wgs} {threads} 0 ms_mlp_fused_kernel<{targs}, %s>"}


def mlp_pre2(c, s1):
    """BN1(s1 W1^T) in float64 on SN1's spikes (ntok, C) in (b, t, hw) row order, cast to fp32 as (D, B HW, Ch)"""
    h = (s1.double() @ c["fc1"]["held"].t()) * c["fc1"]["alpha"].double() + c["fc1"]["beta"].double()
    return h.view(c["B"], c["D"], c["H"] * c["W"], c["Ch"]).permute(1, 0, 2, 3).reshape(c["D"], -1, c["Ch"]).float().contiguous()


def mlp_steps(c, s2):
    """(ntok, Ch) spikes in (b, t, hw) row order -> (D, B HW, Ch)"""
    return s2.view(c["B"], c["D"], c["H"] * c["W"], c["Ch"]).permute(1, 0, 2, 3).reshape(c["D"], -1, c["Ch"]).contiguous()


def mlp_check(c, s1, s2, xo):
    """The three steps on the kernel's own upstream spikes (test_ms_mlp_fused_gpu.py): SN1 bit-equal, SN2 delta-consistent, the output
    x + BN2(s2 W2^T) to 1e-5 of its range.  -> SN2's report"""
    assert torch.equal(s1, c["s1"]), f"SN1 differs from the oracle in {int((s1 != c['s1']).sum())} of {s1.numel()} spikes"
    rep = check_report(c["sn2"].report(mlp_pre2(c, s1), mlp_steps(c, s2)), flips=True)
    check_rate(s2)
    ref = c["x"].reshape(c["ntok"], c["C"]).double() + (s2.double() @ c["fc2"]["held"].t()) * c["fc2"]["alpha"].double() + c["fc2"]["beta"].double()
    err = (xo.reshape(c["ntok"], c["C"]).double() - ref).abs().max().item()
    assert err <= RANGE_TOL * ref.abs().max().item(), err
    return rep


# ---------------------------------------------------------------------------------------------------- 5. token gate
GATE_ROWS = 301                                           # rows x C / 32 lanes is no multiple of 256 for C = 32, 96, 192; two workgroups and more
GATE_VTH = {"lif": 5.0, "plif": 4.0, "lif_hard": 5.5, "lif_vr": 5.0, "lif_tau3": 3.5, "if": 12.0, "psn": 0.0}
GATE_GUARD = 64


@functools.lru_cache(maxsize=None)
def gate_case(Tq, name, Cc):
    """q at rate 0.3 (head sums around 9.6), k at rate 0.5, (Tq, rows, C) u8; e = k AND gate"""
    rows, nH = GATE_ROWS, Cc // 32
    q, k = G.spikes((Tq, rows, Cc), 7700 + Tq + Cc), G.spikes((Tq, rows, Cc), 7701 + Tq + Cc, 0.5)
    sn = neuron(name, GATE_VTH[name], Tq, 30, centre=9.6)
    gate = sn.ref(q.float().view(Tq, rows, nH, 32).sum(3).contiguous())
    e = (k.view(Tq, rows, nH, 32).float() * gate[..., None]).view(Tq, rows, Cc).to(torch.uint8)
    return {"Tq": Tq, "rows": rows, "Cc": Cc, "q": q, "k": k, "sn": sn, "gate": gate, "e": e,
            "route": [f"{-(-rows * nH // 256)} 256 0 qk_gate_kernel"]}
