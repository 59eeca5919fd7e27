"""Inputs, float64 references and buffer layouts of tests/test_spike_gemm_routes_gpu.py (plain CPU code, no GPU call in here).

Every builder is cached: the routes of the test file share one reference per shape, and nothing mutates what a builder returned.

Two kinds of operands:
  exact   weights s * 2^e * (1 + 2^-9 + 2^-17) (one bf16 plane: s * 2^e * (1 + 2^-7)), s = +-1, e in {-2, -1, 0}, and at most 16
          ones per row of A: every partial sum of a row, in any order, is a multiple of 2^-19 below 2^5 - 24 bits - so fp32
          accumulation is exact and the float64 product IS the fp32 result.  The three-term significand needs all three bf16 planes
          (1, 2^-9, 2^-17 after the ties-to-even split) and both fp16 planes ((1 + 2^-9) and 2^-17, normal under the 2^14 scale).
  random  the project's generator: spikes at rate 0.3, |w| <= 0.3 (rounded to bf16 first for the one-plane format, so the
          reference sees the weights the kernel sees); one row of A is silent, so its outputs have no term at all.
"""
import functools

import numpy as np
import torch

from oracle import neuron_ref as R
from oracle import sdformer_oracle as O
from sdformerflow_amd.synthetic import synth_uniform as rnd

GUARD = 64             # guard rows on each side of an output
PAD = 16               # guard columns on each side of an output with ldo > N; bytes in front of / behind an A row with lda > K
V_TH, TAU = 0.1, 2.0   # the neuron of the random fused-neuron cases (the YAML's threshold)
DELTA_ULPS = 16.0      # tests/replay.py
M3 = 1.0 + 2.0 ** -9 + 2.0 ** -17
M1 = 1.0 + 2.0 ** -7


def spikes(shape, seed, rate=0.3):
    return (rnd(shape, seed, 0.0, 1.0) < rate).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def weights(N, K, one_plane, exact):
    """(N, K) fp32.  ns = 2 and ns = 3 share a matrix; ns = 1 has its own (exactly one bf16 plane wide)."""
    if exact:
        g = np.random.Generator(np.random.PCG64(4100 + 7 * N + K))
        s, e = g.integers(0, 2, (N, K)) * 2.0 - 1.0, g.integers(-2, 1, (N, K))
        W = torch.from_numpy((s * 2.0 ** e * (M1 if one_plane else M3)).astype(np.float32))
        W[0, 0] = M1 if one_plane else M3                                  # max |w| in [1, 2): the fp16 scale is 2^14
        return W
    W = rnd((N, K), 4200 + 7 * N + K, -0.3, 0.3)
    return W.bfloat16().float() if one_plane else W


@functools.lru_cache(maxsize=None)
def operand(M, K, exact):
    """(M, K) u8 spikes."""
    if exact:
        g = np.random.Generator(np.random.PCG64(4300 + 3 * M + K))
        A = np.zeros((M, K), np.uint8)
        A[np.arange(M)[:, None], g.integers(0, K, (M, 16))] = 1            # <= 16 ones per row
        return torch.from_numpy(A)
    A = spikes((M, K), 4400 + 3 * M + K)
    if M > 2:
        A[M // 2] = 0                                                      # a silent row: mag = 0 without bias / BN / residual
    return A


# ---------------------------------------------------------------------------------------------------- fp32 epilogue
FLAGS = {"plain": (), "bias": ("bias",), "bn": ("bn",), "res_in": ("res_in",), "res_sep": ("res_sep",), "map": ("map",), "ldo": ("ldo",),
         "lda": ("lda",), "all": ("bias", "bn", "res_in", "map", "ldo", "lda"), "sk_all": ("bias", "bn", "res_sep", "map")}


def scramble(E, zg):
    """Z (M, K) of the head scramble zg = (nH, Tq, B_, N1[, rep]) on E (Tq, B_, N1, nH * 32): O.z_gather_table, inside every replica of
    `rep` windows when given (include/sdformerflow_hip.h, SdfSpikeGemmDesc.zg_rep)."""
    nH, Tq, B_, N1 = zg[:4]
    rep = zg[4] if len(zg) > 4 and zg[4] > 0 else B_
    tab = torch.from_numpy(O.z_gather_table(rep, nH, Tq, N1, 32)).reshape(-1)
    Z = torch.empty_like(E)
    for r in range(B_ // rep):
        sub = E[:, r * rep:(r + 1) * rep].contiguous()
        Z[:, r * rep:(r + 1) * rep] = sub.reshape(-1)[tab].view(Tq, rep, N1, nH * 32)
    return Z.reshape(-1, nH * 32)


@functools.lru_cache(maxsize=None)
def f32_case(M, N, K, one_plane, exact, feat="plain", zg=None):
    """One product with the fp32 epilogue: inputs as the kernel gets them, y (M, N) float64 in the order bias -> BN -> residual, mag
    (M, N) = |alpha| (A |W|^T + |bias|) + |beta| + |resid|, and dst (M,) = the output row of product row m (-1: dropped)."""
    f = FLAGS[feat]
    W = weights(N, K, one_plane, exact)
    if zg is not None:
        E = spikes((zg[1], zg[2], zg[3], K), 4500 + M + K)
        a_dev, A = E.reshape(M, K), scramble(E, zg)
    else:
        a_dev = A = operand(M, K, exact)
    seed = 4600 + 3 * M + 5 * N + K
    y, mag = A.double() @ W.double().t(), A.double() @ W.double().abs().t()
    c = {"M": M, "N": N, "K": K, "flags": f, "W": W, "A": a_dev, "zg": zg, "bias": None, "alpha": None, "beta": None, "resid": None}
    if "bias" in f:
        c["bias"] = rnd((N,), seed + 1, -0.1, 0.1)
        y, mag = y + c["bias"].double(), mag + c["bias"].double().abs()
    if "bn" in f:
        c["alpha"], c["beta"] = rnd((N,), seed + 2, 0.5, 1.5), rnd((N,), seed + 3, -0.2, 0.2)
        y, mag = y * c["alpha"].double() + c["beta"].double(), mag * c["alpha"].double().abs() + c["beta"].double().abs()
    rows = M + 50 if "map" in f else M
    dst = torch.arange(M)
    if "map" in f:                                                         # a permutation into a larger buffer, every seventh row dropped
        dst = torch.randperm(rows, generator=torch.Generator().manual_seed(seed))[:M]
        dst[::7] = -1
    if "res_in" in f or "res_sep" in f:
        c["resid"] = rnd((rows, N), seed + 4, -1.0, 1.0)
        r = c["resid"].double()[dst.clamp(min=0)]
        y, mag = y + r, mag + r.abs()
    c.update(y=y, mag=mag, dst=dst, rows=rows)
    return c


def f32_layout(c):
    """The guarded output of a case -> dict(init (rows_total, ld) fp32 as it is before the call, written (same shape, bool), ref / mag
    (same shape, float64, meaningful where written), ld, c0 = first column of `out`, resid (the separate residual buffer or None))."""
    f, N, rows = c["flags"], c["N"], c["rows"]
    c0 = PAD if "ldo" in f else 0
    ld = N + 2 * c0
    shape = (GUARD + rows + GUARD, ld)
    init = torch.full(shape, float("nan"))
    resid = None
    if "res_in" in f:
        init[GUARD:GUARD + rows, c0:c0 + N] = c["resid"]
    if "res_sep" in f:
        resid = torch.zeros(shape)
        resid[GUARD:GUARD + rows, c0:c0 + N] = c["resid"]
    keep = c["dst"] >= 0
    at = GUARD + c["dst"][keep]
    written, ref, mag = torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    written[at, c0:c0 + N] = True
    ref[at, c0:c0 + N] = c["y"][keep]
    mag[at, c0:c0 + N] = c["mag"][keep]
    return {"init": init, "written": written, "ref": ref, "mag": mag, "ld": ld, "c0": c0, "resid": resid}


def a_layout(c):
    """(buffer, first byte of A in it, lda): A as it is, or - lda > K - a column slice of a wider byte matrix of ones."""
    A, K = c["A"], c["K"]
    if "lda" not in c["flags"]:
        return A.contiguous(), 0, K
    wide = torch.ones((A.shape[0], K + 2 * PAD), dtype=torch.uint8)
    wide[:, PAD:PAD + K] = A
    return wide, PAD, K + 2 * PAD


# ---------------------------------------------------------------------------------------------------- fused neuron
KINDS = {"lif": ("lif", None), "lif0": ("lif", 0.0), "if": ("if", None), "psn": ("psn", None)}     # name -> (neuron, v_reset)


# seeds are chosen so that the REFERENCE's own decisions stay under the cap on ambiguous ones (at most 1e-4 of a case's decisions within
# delta of the threshold; the CPU test of the routes file asserts it): the small cases allow not a single one
RESEED = {(5, 25, 64, 160): 1000}


def sn_rows(h, T, pos, layout):
    """Rows in the kernel's order -> (T, pos, N).  tm: time-major rows (t, position) - addressing (pos, pos, 0, pos); bt: rows
    (b, t, hw) with b < 2 - addressing (2 HW, HW, T HW, HW)."""
    if layout == "tm":
        return h.view(T, pos, -1)
    return h.view(2, T, pos // 2, -1).permute(1, 0, 2, 3).reshape(T, pos, -1)


def sn_addressing(T, pos, layout):
    """(pos_count, pos_inner, pos_ostride, t_stride)"""
    return (pos, pos, 0, pos) if layout == "tm" else (pos, pos // 2, T * (pos // 2), pos // 2)


@functools.lru_cache(maxsize=None)
def sn_case(T, pos, N, K, one_plane, kind, layout):
    """A random fused-neuron case: BN, the positional term with add_prows = 7, the neuron `kind` at v_th = 0.1, tau = 2.  x = the
    float64 pre-activation (T, pos, N) cast to fp32; delta = 16 * 2^-23 * max(rms(x), v_th)."""
    W = weights(N, K, one_plane, False)
    seed = 4700 + 11 * T + 3 * pos + N + K + RESEED.get((T, pos, N, K), 0)
    A = spikes((T * pos, K), seed)
    alpha, beta, add = rnd((N,), seed + 1, 0.5, 1.5), rnd((N,), seed + 2, -0.2, 0.2), rnd((T, 7, N), seed + 3, -0.3, 0.3)
    h = sn_rows((A.double() @ W.double().t()) * alpha.double() + beta.double(), T, pos, layout)
    x = (h + add.double()[:, torch.arange(pos) % 7]).float().contiguous()
    neuron, v_reset = KINDS[kind]
    Wn, bn = rnd((T, T), seed + 4, -0.5, 0.5) + 0.5 * torch.eye(T), torch.full((T,), -0.1)
    delta = DELTA_ULPS * 2.0 ** -23 * max(float(x.double().pow(2).mean().sqrt()), V_TH)
    return {"T": T, "pos": pos, "N": N, "K": K, "W": W, "A": A, "alpha": alpha, "beta": beta, "add": add, "x": x, "delta": delta,
            "neuron": neuron, "v_reset": v_reset, "v_th": V_TH, "psn_w": Wn, "psn_b": bn, "layout": layout,
            "ncfg": O.NeuronCfg(neuron, V_TH, v_reset, TAU, T), "sd": {"w.weight": Wn, "w.bias": bn}}


def sn_reference(c):
    """The reference neuron's own spikes (T, pos, N) for a case's x."""
    return R.neuron_ref(c["x"], c["neuron"], TAU, c["v_th"], c["v_reset"], psn_w=c["psn_w"], psn_b=c["psn_b"])


def sn_report(c, got):
    """O.delta_consistent of spikes `got` (T, pos, N) for a random case."""
    return O.delta_consistent(c["x"], got.float(), c["ncfg"], c["sd"], "w.", c["delta"])


@functools.lru_cache(maxsize=None)
def sn_exact_case(T, pos, N, K, one_plane, kind, layout):
    """A fused-neuron case on the exact operands, no BN, no positional term: the pre-activation is c * m with c a multiple of 1/4 and
    m the weights' significand, exact in fp32 in any order, and the threshold is m itself (LIF, tau = 2: the first charge is x / 2, so
    c = 2 sits ON the threshold; PSN with W = I + subdiagonal / 2 and bias -m: c_t + c_(t-1) / 2 = 1 does).  The neuron's arithmetic is
    the reference's op sequence, so the spikes must EQUAL the reference's - decisions on the threshold included, which is what
    tells `>` from `>=`."""
    m = M1 if one_plane else M3
    W = weights(N, K, one_plane, True)
    A = operand(T * pos, K, True)
    x = sn_rows(A.double() @ W.double().t(), T, pos, layout)
    neuron, v_reset = KINDS[kind]
    Wn = torch.eye(T) + 0.5 * torch.diag(torch.ones(T - 1), -1)
    c = {"T": T, "pos": pos, "N": N, "K": K, "W": W, "A": A, "alpha": None, "beta": None, "add": None, "x64": x, "x": x.float().contiguous(),
         "neuron": neuron, "v_reset": v_reset, "v_th": m, "psn_w": Wn, "psn_b": torch.full((T,), -m), "layout": layout}
    return c


def on_threshold(c):
    """Number of first-step decisions of an exact case whose membrane is exactly the threshold."""
    x0 = c["x"][0].double()
    if c["neuron"] == "psn":
        return int((x0 == c["v_th"]).sum())
    return int(((x0 if c["neuron"] == "if" else x0 / 2) == float(np.float32(c["v_th"]))).sum())
