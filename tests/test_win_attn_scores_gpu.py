"""The attention map (B_, nH, N, N) of the window attention (csrc/win_attn_scores.hip, sdf_win_attn_scores_fwd: win_attn_scores_kernel,
one design for 1 <= N <= 1024, keys walked in blocks of 64, twice in the ANN mode) against the second return value of the oracle's
matrix cores (oracle.sdformer_oracle.ann_attention_core / sew_attention_core) evaluated in float64 on the same fp32 / byte inputs -
the method of tests/test_win_attn_large_gpu.py, restated.  Every case

  * asserts through hip.launch_log() that exactly ONE launch happened and that it was win_attn_scores_kernel with the expected mode and
    mask flag in its template arguments, one workgroup of 256 threads per (window, head, 64 queries);
  * hands the kernel a `scores` that is a slice of a larger buffer, 61 guard elements on each side (so the map starts on a 4-byte
    boundary only), everything NaN beforehand: the guards must still hold the same NaN bits and no NaN may remain inside;
  * runs the call twice: bit-equal results.

Sizes (nH = 3): 18 (window (2,3,3): less than one key block and one query block), 162 (the shipped window), 194 (the first size past
the first forward entry point's 192: a 2-key tail; SEW Tq 2 x N1 97), 225 (odd: rows are only 4-byte aligned, a 1-key tail; SEW as
Tq 3 x N1 75), 450 (the (2,15,15) window with its real shift mask: 8 key blocks, the last with 2 of 64 keys) and 1024 (the ceiling).

Bounds.  ANN - the project's own: 2e-5 is what tests/test_win_attn_fwd_gpu.py and tests/test_win_attn_large_gpu.py put on P @ v with
|v| <= 1; a single probability is that output for a one-hot v and a row sum that output for v = 1, so max |p - p64| <= 2e-5 and
max |sum_j p - 1| <= 2e-5.  The recipe's logits are large (bias up to 14, logit scale up to 100), so a key wrongly admitted past N
with logit 0 would weigh e^-14 and pass; the `low` cases repeat the ragged shapes with |logit| <= 5.5, where it would carry a
visible share of the row.  SEW - derived: the count c of common spikes is exact; three fp32 roundings follow (two with an fma), each
at most 2^-24 of a magnitude no larger than S = c * scale + |bias| + |mask|, so |a - a64| <= 2^-22 * S per element, scale being the
fp32 value the kernel reads.  With a zero bias and no mask the map is fp32(c * scale), bit for bit.

Largest error measured on an MI355X (all cases of this file):
  ANN, max |p - p64|:      6.2e-6 (N = 194 with a mask; 5.1e-6 at N = 1024, 4.9e-6 windowed with padding tokens, 3.8e-6 at N = 450 with
                           the shift mask, 1.3e-7 with small logits); max |sum_j p - 1|: 3.4e-7 (N = 1024)
  SEW, max |a - a64| / S:  8.4e-8 (N = 1024; 7.6e-8 .. 8.4e-8 at every size) against 2^-22 = 2.4e-7
  fixtures:                ANN attn00 9.2e-7; SEW attn00 7.6e-6 (lif), 0 (psn: scale 1, integer scores), map sums 0.22 / 0.17
Run time there: the 29 cases of this file in 2.8 s together."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import sdformer_oracle as O
from sdformerflow_amd import hip
from sdformerflow_amd.synthetic import synth_state_dict, synth_uniform as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 61                                       # guard elements on each side of `scores` (odd: the map is 4-byte aligned only)
ANN_TOL = 2e-5
SEW_REL = 2.0 ** -22
KERNEL = "win_attn_scores_kernel"
NH = 3
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _assert_one_launch(log, mode, N, masked, B_, nH):
    """Exactly one launch, of win_attn_scores_kernel<mode, mask>, one workgroup of 256 threads per (window, head, 64 queries)."""
    assert len(log.rows) == 1, log.rows
    name, wgs, threads, lds, _ = log.rows[0]
    m = int(mode == "sew")
    want = (f"{KERNEL}<{m}, {'true' if masked else 'false'}>", f"{KERNEL}ILi{m}ELb{int(masked)}EE")
    assert want["<" not in name] in name, (name, want)           # demangled, or the mangled name when the demangler gave up
    groups = ((N + 15) // 16 + 3) // 4
    assert wgs == B_ * nH * groups and threads == 256 and lds == 0      # (its 9 KiB of LDS are static)
    return name


def _mask(N, nW, seed):
    """(nW, N, N) 0 / -100: the shifted-window mask of the (2,15,15) window, else from random labels in {0, 1, 2} per window
    (-100 where the labels differ: the diagonal is 0, no row is fully masked)."""
    if (N, nW) == (450, 4):
        return O.compute_mask(2, 30, 30, (2, 15, 15), (1, 7, 7))
    lab = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).integers(0, 3, (nW, N)))
    return torch.where(lab[:, :, None] != lab[:, None, :], torch.tensor(-100.0), torch.tensor(0.0))


def _ann_params(nH, N, seed, low=False):
    """(logit_scale (nH,1,1), bias (nH,N,N)): head 0 at exactly 100 (the largest logits carry the largest error); low: |logit| <=
    e^1.5 + 1."""
    if low:
        return torch.full((nH, 1, 1), math.exp(1.5)), rnd((nH, N, N), seed + 2, -1.0, 1.0)
    ls = torch.exp(torch.clamp(rnd((nH, 1, 1), seed + 1, 1.5, 5.0), max=math.log(100.0)))
    ls[0] = 100.0
    return ls, 16 * torch.sigmoid(rnd((nH, N, N), seed + 2, -2.0, 2.0))


@functools.lru_cache(maxsize=None)
def _ann_case(N, B_, nH, nW, masked, low=False):
    """Inputs and the fp64 probabilities (B_, nH, N, N) of one ANN case."""
    seed = 27000 + 16 * N + int(masked) + 2 * int(low)
    qkv = rnd((B_, N, 3 * nH * 32), seed, -1.0, 1.0)
    ls, bias = _ann_params(nH, N, seed, low)
    mask = _mask(N, nW, seed + 3) if masked else None
    _, p = O.ann_attention_core(qkv.double(), ls.double(), bias.double(), mask.double() if masked else None, nH)
    return qkv, ls, bias, mask, p


@functools.lru_cache(maxsize=None)
def _sew_case(Tq, N1, B_, nH, nW, masked, zero_bias_head=None):
    """Inputs, the fp64 scores (B_, nH, N, N), the per-element bound 2^-22 * (c * scale + |bias| + |mask|) and the counts c of one
    SEW case."""
    N, Cc = Tq * N1, nH * 32
    seed = 29000 + 16 * N + int(masked)
    spk = lambda s, rate: (rnd((Tq, B_, N1, Cc), s, 0.0, 1.0) < rate).to(torch.uint8)
    q, k = spk(seed, 0.3), spk(seed + 1, 0.4)
    bias = rnd((nH, N, N), seed + 3, -1.0, 1.0)
    if zero_bias_head is not None:
        bias[zero_bias_head] = 0.0
    mask = _mask(N, nW, seed + 4) if masked else None
    scale = torch.full((nH,), 32 ** -0.5)                                        # fp32, as the kernel reads it
    view = lambda t: t.double().reshape(B_, nH, N, 32)                           # the reference's raw head view
    _, attn = O.sew_attention_core(view(q), view(k), view(k), float(scale[0]), bias.double(), mask.double() if masked else None, Tq, N1)
    c = view(q) @ view(k).transpose(-2, -1)
    S = c * float(scale[0]) + bias.double().abs().unsqueeze(0)
    if masked:
        S = (S.view(B_ // nW, nW, nH, N, N) + mask.double().abs().view(1, nW, 1, N, N)).view(B_, nH, N, N)
    return q, k, scale, bias, mask, attn, SEW_REL * S, c


def _launch(fill, B_, nH, N):
    """One sdf_win_attn_scores_fwd call into a NaN-filled, guarded buffer -> (map (B_, nH, N, N) on the CPU, launch log)."""
    n = B_ * nH * N * N
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    nan_bits = int(bits[0])
    d = hip.WinAttnDesc()
    fill(d)
    with hip.launch_log() as log:
        rc = hip.lib().sdf_win_attn_scores_fwd(ctypes.byref(d), buf[GUARD:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((bits[:GUARD] == nan_bits).all()) and bool((bits[GUARD + n:] == nan_bits).all()), "a store outside `scores`"
    return buf[GUARD:GUARD + n].cpu().view(B_, nH, N, N), log


def _dev(*ts):
    return [None if t is None else t.contiguous().to(DEV) for t in ts]


def _run_ann(case, nH, nW, row_map=None, pad=None, B_=None, N=None):
    qkv, ls, bias, mask = case
    if row_map is None:
        B_, N = qkv.shape[:2]
    t = _dev(qkv, ls.reshape(-1), bias, mask, pad)

    def fill(d):                                                                  # (k, v and out stay NULL: ignored in this mode)
        d.mode, d.q = 0, t[0].data_ptr()
        d.B_, d.nW, d.nH, d.N, d.hd = B_, (nW if mask is not None else 1), nH, N, 32
        d.scale, d.bias, d.mask = t[1].data_ptr(), t[2].data_ptr(), (t[3].data_ptr() if mask is not None else None)
        if row_map is not None:
            d.row_map, d.pad_qkv = row_map.data_ptr(), t[4].data_ptr()
    return _launch(fill, B_, nH, N)


def _run_sew(case, Tq, N1, B_, nH, nW):
    q, k, scale, bias, mask = case
    t = _dev(q, k, scale, bias, mask)

    def fill(d):                                                                  # (v and out stay NULL)
        d.mode, d.q, d.k = 1, t[0].data_ptr(), t[1].data_ptr()
        d.B_, d.nW, d.nH, d.N, d.hd, d.Tq, d.N1 = B_, (nW if mask is not None else 1), nH, Tq * N1, 32, Tq, N1
        d.scale, d.bias, d.mask = t[2].data_ptr(), t[3].data_ptr(), (t[4].data_ptr() if mask is not None else None)
    return _launch(fill, B_, nH, Tq * N1)


def _check_ann(run, ref, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, "ann", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an element of the map was never written"
    err = (got.double() - ref).abs().max().item()
    serr = (got.double().sum(-1) - 1.0).abs().max().item()
    print(f"\nWINATTN_SCORES ann {what} err {err:.3e} rowsum {serr:.3e}  [{name}]")
    assert err <= ANN_TOL, err
    assert serr <= ANN_TOL, serr
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"
    return got


def _check_sew(run, ref, bound, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, "sew", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an element of the map was never written"
    err = (got.double() - ref).abs()
    nz = bound > 0
    rel = (err[nz] / bound[nz]).max().item() * SEW_REL if bool(nz.any()) else 0.0
    print(f"\nWINATTN_SCORES sew {what} err/S {rel:.3e}  [{name}]")
    assert bool((err <= bound).all()), rel
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"
    return got


# (N, SEW Tq, masked): B_ = nW = 4 with a mask, B_ = 1 without
CASES = [(18, 2, True), (18, 2, False), (162, 2, True), (162, 2, False), (194, 2, True), (194, 2, False), (225, 3, True), (225, 3, False),
         (450, 2, True), (1024, 2, False)]
IDS = [f"N{n}-{'mask' if m else 'nomask'}" for n, _, m in CASES]


@pytest.mark.parametrize("N,Tq,masked", CASES, ids=IDS)
def test_ann_map(N, Tq, masked):
    B_ = nW = 4 if masked else 1
    *case, ref = _ann_case(N, B_, NH, nW, masked)
    _check_ann(lambda: _run_ann(case, NH, nW), ref, N, masked, B_, NH, f"N={N} mask={masked}")


@pytest.mark.parametrize("N,Tq,masked", CASES, ids=IDS)
def test_sew_map(N, Tq, masked):
    B_ = nW = 4 if masked else 1
    *case, ref, bound, _ = _sew_case(Tq, N // Tq, B_, NH, nW, masked)
    _check_sew(lambda: _run_sew(case, Tq, N // Tq, B_, NH, nW), ref, bound, N, masked, B_, NH, f"N={N} Tq={Tq} mask={masked}")


@pytest.mark.parametrize("N", [194, 225, 450])
def test_ann_ragged_tail_with_small_logits(N):
    """The ragged shapes again with |logit| <= 5.5 (and the mask): a key past N admitted with logit 0 now carries a visible share of
    a row's weight instead of e^-14 (the row sum and every probability of the row would move by > 2e-4 / N ... 1 / N)."""
    *case, ref = _ann_case(N, 4, NH, 4, True, low=True)
    _check_ann(lambda: _run_ann(case, NH, 4), ref, N, True, 4, NH, f"N={N} low logits")


def test_sew_zero_bias_head_is_the_scaled_count_bit_for_bit():
    """No mask and a zero bias on head 1: there the element is fp32(c * scale) exactly - c the count of common spikes, an integer
    the fp32 MFMA accumulates without rounding - and (that + 0) changes nothing."""
    N, Tq, B_ = 225, 3, 1
    *case, ref, bound, c = _sew_case(Tq, N // Tq, B_, NH, 1, False, zero_bias_head=1)
    got = _check_sew(lambda: _run_sew(case, Tq, N // Tq, B_, NH, 1), ref, bound, N, False, B_, NH, "N=225 zero bias on head 1")
    scale = case[2]
    assert c.max() >= 8 and torch.equal(c, c.round())
    assert torch.equal(got[:, 1], c[:, 1].float() * scale[1])


# ---------------------------------------------------------------- the window partition inside the kernel
B_W, D_W, H_W, W_W, WS, SS = 1, 4, 20, 33, (2, 15, 15), (1, 7, 7)


@functools.lru_cache(maxsize=None)
def _windowed_case():
    """fp64 through the oracle's slice table (pad + roll + window partition as one index table, -1 = padding token, which reads the
    `pad` row): gather -> ann_attention_core's probabilities, padding tokens as rows and columns."""
    Cc, seed, N = NH * 32, 31000, WS[0] * WS[1] * WS[2]
    rows = B_W * D_W * H_W * W_W
    qkv = rnd((rows, 3 * Cc), seed, -1.0, 1.0)
    pad = rnd((3 * Cc,), seed + 4, -1.0, 1.0)
    ls, bias = _ann_params(NH, N, seed)
    Dp, Hp, Wp = D_W + (-D_W) % WS[0], H_W + (-H_W) % WS[1], W_W + (-W_W) % WS[2]
    mask = O.compute_mask(Dp, Hp, Wp, WS, SS)
    src, B_ = O.slice_table(B_W, D_W, H_W, W_W, WS, SS)             # (B_ * Wd, Wh * Ww): window-major, then the in-window frame
    src = torch.from_numpy(src).reshape(B_, N)
    flat = torch.cat([qkv.double(), pad.double()[None]], 0)
    win = flat[torch.where(src < 0, torch.tensor(rows), src)]       # (B_, N, 3C)
    _, p = O.ann_attention_core(win, ls.double(), bias.double(), mask.double(), NH)
    return qkv, ls, bias, mask, pad, p, B_, src


def test_ann_windowed_map_at_450_tokens():
    """The (2,15,15) window with shift (1,7,7) on a (1, 4, 20, 33) map: 30 x 45 padded, so every window holds padding tokens, which
    read pad_qkv and ARE rows and columns of the map; row_map from hip.window_slice_map, equal to the oracle's table."""
    qkv, ls, bias, mask, pad, ref, B_, src = _windowed_case()
    N = 450
    row_map, B2 = hip.window_slice_map(B_W, D_W, H_W, W_W, WS, SS, DEV)
    assert B2 == B_ == 12 == mask.shape[0] and torch.equal(row_map.cpu().view(B_, N).long(), src)
    assert bool((src < 0).view(B_, 2, 15, 15).any(-1).any(-1).all())                     # padding tokens in every window
    run = lambda: _run_ann((qkv, ls, bias, mask), NH, B_, row_map=row_map, pad=pad, B_=B_, N=N)
    _check_ann(run, ref, N, True, B_, NH, "windowed (2,15,15) shift (1,7,7)")


# ---------------------------------------------------------------- the real reference's fixtures
def _sew_shapes(C, nH, kind, T=2):
    s = {"relative_position_bias_table": (3 * 17 * 17, nH), "proj.weight": (C, C), "proj.bias": (C,)}
    for n in ("q", "k", "v"):
        s[f"linear_{n}.weight"] = (C, C)
    for bn in ("bn_q", "bn_k", "bn_v", "proj_bn"):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            s[f"{bn}.norm_layer.{leaf}"] = (C,)
    if kind == "psn":
        for sn in ("sn_q", "sn_k", "sn_v", "attn_sn", "proj_sn"):
            s[f"{sn}.spiking_neuron.weight"] = (T, T)
            s[f"{sn}.spiking_neuron.bias"] = (T, 1)
    return s


def test_ann_map_equals_the_reference_fixture():
    """tests/golden/ann_attention.npz `attn00` (the real WindowAttention3D's second value, window 0, head 0) on the inputs
    tests/test_oracle_golden.py builds for it; the qkv projection is the oracle's, on the CPU."""
    g = np.load(os.path.join(GOLDEN, "ann_attention.npz"))
    C, nH, nW, ws = 96, 3, 4, (2, 9, 9)
    shapes = {"logit_scale": (nH, 1, 1), "cpb_mlp.0.weight": (512, 3), "cpb_mlp.0.bias": (512,), "cpb_mlp.2.weight": (nH, 512),
              "qkv.weight": (3 * C, C), "qkv.bias": (3 * C,), "proj.weight": (C, C), "proj.bias": (C,)}
    sd = synth_state_dict(shapes)
    x = rnd((nW, 162, C), 13, -1.0, 1.0)
    mask = O.compute_mask(2, 18, 18, ws, (1, 4, 4))
    qkv = O._lin(x, sd["qkv.weight"], sd["qkv.bias"])
    ls = torch.clamp(sd["logit_scale"], max=math.log(1.0 / 0.01)).exp()
    got, log = _run_ann((qkv, ls, O.ann_cpb_bias(sd, "", nH, ws), mask), nH, nW)
    _assert_one_launch(log, "ann", 162, True, nW, nH)
    err = np.abs(got[0, 0].numpy().astype(np.float64) - g["attn00"]).max()
    print(f"\nWINATTN_SCORES ann fixture attn00 err {err:.3e}")
    assert err <= ANN_TOL, err


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_sew_map_equals_the_reference_fixture(kind):
    """tests/golden/sew_attention.npz `<kind>_attn00` / `<kind>_attn_sum` (the real Spiking_BN_WindowAttention3D's second value) on the
    inputs tests/test_oracle_golden.py builds for them, to the numbers that file holds the oracle to (1e-4, 0.5).  The q and k
    spikes are the oracle's CPU run (Linear -> BN -> neuron), so no spike decision is re-made on the GPU."""
    g = np.load(os.path.join(GOLDEN, "sew_attention.npz"))
    C, nH, B, nW, ws = 96, 3, 2, 4, (2, 9, 9)
    sd = synth_state_dict(_sew_shapes(C, nH, kind))
    x = (rnd((2, B * nW, 9, 9, C), 11) > 0.4).float().reshape(2, B * nW, 81, C)
    mask = O.compute_mask(2, 18, 18, ws, (1, 4, 4))
    ncfg = O.NeuronCfg(kind, v_th=0.1, v_reset=None, tau=2.0, num_steps=2)
    spikes = lambda n: O.neuron(O.bn_last(O._lin(x, sd[f"linear_{n}.weight"]), sd, f"bn_{n}.norm_layer."), ncfg, sd,
                                f"sn_{n}.spiking_neuron.").to(torch.uint8)
    idx = torch.from_numpy(O.relative_position_index(ws).reshape(-1))
    bias = sd["relative_position_bias_table"][idx].reshape(162, 162, nH).permute(2, 0, 1).contiguous()
    scale = torch.full((nH,), 1.0 if kind == "psn" else 32 ** -0.5)                # reference :240-243
    got, log = _run_sew((spikes("q"), spikes("k"), scale, bias, mask), 2, 81, B * nW, nH, nW)
    _assert_one_launch(log, "sew", 162, True, B * nW, nH)
    e00 = np.abs(got[0, 0].numpy() - g[f"{kind}_attn00"]).max()
    esum = np.abs(got.double().sum((-1, -2)).numpy() - g[f"{kind}_attn_sum"]).max()
    print(f"\nWINATTN_SCORES sew fixture {kind} attn00 err {e00:.3e} sum err {esum:.3e}")
    assert e00 <= 1e-4, e00
    assert esum <= 0.5, esum


# ---------------------------------------------------------------- wrappers
def test_wrappers_run_the_same_call_and_refuse_beyond_1024():
    """hip.win_attn_ann_scores / win_attn_sew_scores fill the descriptor as this file does: bit-equal results; 1025 tokens raise
    SdfError with the library's E_SHAPE before any launch."""
    N, B_, nW = 194, 4, 4
    qkv, ls, bias, mask, _ = _ann_case(N, B_, NH, nW, True)
    got, _ = _run_ann((qkv, ls, bias, mask), NH, nW)
    t = _dev(qkv, ls.reshape(-1), bias, mask)
    with hip.launch_log() as log:
        out = hip.win_attn_ann_scores(*t, NH)
    assert len(log.rows) == 1 and KERNEL in log.rows[0][0]
    assert out.shape == (B_, NH, N, N) and out.dtype == torch.float32 and torch.equal(out.cpu(), got)
    q, k, scale, bias, mask, _, _, _ = _sew_case(2, N // 2, B_, NH, nW, True)
    got, _ = _run_sew((q, k, scale, bias, mask), 2, N // 2, B_, NH, nW)
    t = _dev(q, k, scale, bias, mask)
    out = hip.win_attn_sew_scores(*t, NH, 2, B_, N // 2)
    assert out.shape == (B_, NH, N, N) and torch.equal(out.cpu(), got)
    qkv, ls, bias, mask, pad, _, B_, _ = _windowed_case()
    row_map, _ = hip.window_slice_map(B_W, D_W, H_W, W_W, WS, SS, DEV)
    got, _ = _run_ann((qkv, ls, bias, mask), NH, B_, row_map=row_map, pad=pad, B_=B_, N=450)
    t = _dev(qkv, ls.reshape(-1), bias, mask, pad)
    assert torch.equal(hip.win_attn_ann_scores(t[0], t[1], t[2], t[3], NH, row_map, B_, 450, t[4]).cpu(), got)
    with hip.launch_log() as log, pytest.raises(hip.SdfError) as e:
        hip.win_attn_ann_scores(torch.zeros((1, 1025, 288), device=DEV), torch.ones(3, device=DEV), torch.zeros((3, 8, 8), device=DEV), None, NH)
    assert e.value.rc == hip.E_SHAPE and not log.rows
    with hip.launch_log() as log, pytest.raises(hip.SdfError) as e:
        z = torch.zeros((1, 1, 1025, 96), dtype=torch.uint8, device=DEV)
        hip.win_attn_sew_scores(z, z, torch.ones(3, device=DEV), torch.zeros((3, 8, 8), device=DEV), None, NH, 1, 1, 1025)
    assert e.value.rc == hip.E_SHAPE and not log.rows
