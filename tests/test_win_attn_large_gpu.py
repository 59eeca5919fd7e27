"""Forward of the window attention for 192 < N <= 1024 tokens per window (csrc/win_attn_large.hip, sdf_win_attn_large_fwd:
win_attn_large_kernel, keys walked in blocks of 64, online softmax in the ANN mode) against the oracle's matrix cores
(oracle.sdformer_oracle.ann_attention_core / sew_attention_core) evaluated in float64 on the same fp32 / byte inputs - the method of
tests/test_win_attn_fwd_gpu.py, restated.  Every case

  * asserts through hip.launch_log() that exactly ONE launch happened and that it was win_attn_large_kernel with the expected mode and
    mask flag in its template arguments, one workgroup of 256 threads per (window, head, 64 queries);
  * hands the kernel an `out` that is a slice of a larger buffer, 64 guard rows on each side, everything NaN beforehand: the guards
    must still hold the same NaN bits and no NaN may remain inside;
  * runs the call twice: bit-equal results.

Sizes: 194 (the first even size past the first entry point's limit: 13 key tiles, a 2-key tail in the last; Tq 2 x N1 97), 200, 225 (odd:
bias / mask rows are only 4-byte aligned, a 1-key tail; SEW as Tq 3 x N1 75), 450 (the (2,15,15) window with its real shift mask:
8 key blocks, the last with 2 of 64 keys) and 1024 (the ceiling: 16 whole blocks, 16 workgroups per (window, head)).

Bounds - the project's own, from tests/test_win_attn_fwd_gpu.py.  ANN (cosine softmax, |v| <= 1): max |got - ref64| <= 2e-5.  SEW (no
softmax): per element |got - ref64| <= 1e-5 * (|attn64| @ v) through the same output scramble, and exact equality where that sum is
0.  The recipe's logits are large (bias up to 14, logit scale up to 100), so a key wrongly admitted past the ragged tail with logit 0
would weigh e^-14 and pass; the `low` cases repeat the ragged shapes with |logit| <= 5.5, where such a key weighs > 2e-4 / N.

Largest error measured on an MI355X (all cases of this file):
  ANN, max |got - ref64|:         8.4e-6 (N = 1024; 8.0e-6 at N = 450 with the shift mask, 7.4e-6 windowed, 2.2e-7 with small logits)
  SEW, max |err| / (|attn| @ v):  1.4e-6 (N = 1024; 1.2e-6 at N = 450, 6.4e-7 at N <= 225)
Run time there: the 21 cases of this file in 3.2 s together."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import sdformer_oracle as O
from sdformerflow_amd import hip
from sdformerflow_amd.synthetic import synth_uniform as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                       # guard rows on each side of `out`
ANN_TOL, SEW_TOL = 2e-5, 1e-5
KERNEL = "win_attn_large_kernel"
NH = 3


def _assert_one_launch(log, mode, N, masked, B_, nH):
    """Exactly one launch, of win_attn_large_kernel<mode, mask>, one workgroup of 256 threads per (window, head, 64 queries)."""
    assert len(log.rows) == 1, log.rows
    name, wgs, threads, lds, _ = log.rows[0]
    m = int(mode == "sew")
    want = (f"{KERNEL}<{m}, {'true' if masked else 'false'}>", f"{KERNEL}ILi{m}ELb{int(masked)}EE")
    assert want["<" not in name] in name, (name, want)           # demangled, or the mangled name when the demangler gave up
    groups = ((N + 15) // 16 + 3) // 4
    assert wgs == B_ * nH * groups and threads == 256 and lds == 0      # (its 17.5 KiB of LDS are static)
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
    """Inputs and the fp64 reference of one ANN case."""
    seed = 17000 + 16 * N + int(masked) + 2 * int(low)
    qkv = rnd((B_, N, 3 * nH * 32), seed, -1.0, 1.0)
    ls, bias = _ann_params(nH, N, seed, low)
    mask = _mask(N, nW, seed + 3) if masked else None
    ref, _ = O.ann_attention_core(qkv.double(), ls.double(), bias.double(), mask.double() if masked else None, nH)
    return qkv, ls, bias, mask, ref.reshape(B_ * N, nH * 32)


@functools.lru_cache(maxsize=None)
def _sew_case(Tq, N1, B_, nH, nW, masked):
    """Inputs, the fp64 reference and the per-element bound 1e-5 * (|attn64| @ v) of one SEW case."""
    N, Cc = Tq * N1, nH * 32
    seed = 19000 + 16 * N + int(masked)
    spk = lambda s, rate: (rnd((Tq, B_, N1, Cc), s, 0.0, 1.0) < rate).to(torch.uint8)
    q, k, v = spk(seed, 0.3), spk(seed + 1, 0.4), spk(seed + 2, 0.5)
    v.view(B_, nH, N, 32)[..., 5] = 0                                            # one silent head dim: its outputs are exactly 0
    bias = rnd((nH, N, N), seed + 3, -1.0, 1.0)
    mask = _mask(N, nW, seed + 4) if masked else None
    scale = torch.full((nH,), 32 ** -0.5)                                        # fp32, as the kernel reads it
    view = lambda t: t.double().reshape(B_, nH, N, 32)                           # the reference's raw head view
    ref, attn = O.sew_attention_core(view(q), view(k), view(v), float(scale[0]), bias.double(), mask.double() if masked else None, Tq, N1)
    mag = (attn.abs() @ view(v)).reshape(B_, nH, Tq, N1, 32).permute(2, 0, 3, 1, 4).reshape(Tq * B_ * N1, Cc)
    return q, k, v, scale, bias, mask, ref.reshape(Tq * B_ * N1, Cc), SEW_TOL * mag


def _launch(fill, rows, Cc):
    """One sdf_win_attn_large_fwd call into a NaN-filled, guarded `out` -> (result (rows, Cc) on the CPU, launch log)."""
    buf = torch.full((GUARD + rows + GUARD, Cc), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    nan_bits = int(bits[0, 0])
    d = hip.WinAttnDesc()
    fill(d)
    d.out = buf[GUARD:].data_ptr()
    with hip.launch_log() as log:
        rc = hip.lib().sdf_win_attn_large_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((bits[:GUARD] == nan_bits).all()) and bool((bits[GUARD + rows:] == nan_bits).all()), "a store outside `out`"
    return buf[GUARD:GUARD + rows].cpu(), log


def _dev(*ts):
    return [None if t is None else t.contiguous().to(DEV) for t in ts]


def _run_ann(case, nH, nW, row_map=None, pad=None, B_=None, N=None, rows=None):
    qkv, ls, bias, mask = case
    if row_map is None:
        B_, N = qkv.shape[:2]
        rows = B_ * N
    t = _dev(qkv, ls.reshape(-1), bias, mask, pad)

    def fill(d):
        d.mode, d.q, d.k, d.v = 0, t[0].data_ptr(), t[0].data_ptr(), t[0].data_ptr()
        d.B_, d.nW, d.nH, d.N, d.hd = B_, (nW if mask is not None else 1), nH, N, 32
        d.scale, d.bias, d.mask = t[1].data_ptr(), t[2].data_ptr(), (t[3].data_ptr() if mask is not None else None)
        if row_map is not None:
            d.row_map, d.pad_qkv = row_map.data_ptr(), t[4].data_ptr()
    return _launch(fill, rows, nH * 32)


def _run_sew(case, Tq, N1, B_, nH, nW):
    q, k, v, scale, bias, mask = case
    t = _dev(q, k, v, scale, bias, mask)

    def fill(d):
        d.mode, d.q, d.k, d.v = 1, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
        d.B_, d.nW, d.nH, d.N, d.hd, d.Tq, d.N1 = B_, (nW if mask is not None else 1), nH, Tq * N1, 32, Tq, N1
        d.scale, d.bias, d.mask = t[3].data_ptr(), t[4].data_ptr(), (t[5].data_ptr() if mask is not None else None)
    return _launch(fill, Tq * B_ * N1, nH * 32)


def _check_ann(run, ref, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, "ann", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an output row was never written"
    err = (got.double() - ref).abs().max().item()
    print(f"\nWINATTN_LARGE ann {what} err {err:.3e}  [{name}]")
    assert err <= ANN_TOL, err
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"


def _check_sew(run, ref, bound, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, "sew", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an output row was never written"
    err = (got.double() - ref).abs()
    zero = bound == 0
    rel = (err[~zero] / bound[~zero]).max().item() * SEW_TOL
    print(f"\nWINATTN_LARGE sew {what} err/(|attn|@v) {rel:.3e}  [{name}]")
    assert bool(zero.view(-1, 32)[:, 5].all()) and torch.equal(got[zero].double(), ref[zero]), "an element whose every term is 0 is not exactly 0"
    assert bool((err <= bound).all()), rel
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"


# (N, SEW Tq, masked): B_ = nW = 4 with a mask, B_ = 1 without
CASES = [(194, 2, True), (194, 2, False), (200, 2, True), (200, 2, False), (225, 3, True), (225, 3, False), (450, 2, True), (1024, 2, False)]
IDS = [f"N{n}-{'mask' if m else 'nomask'}" for n, _, m in CASES]


@pytest.mark.parametrize("N,Tq,masked", CASES, ids=IDS)
def test_ann_large_window(N, Tq, masked):
    B_ = nW = 4 if masked else 1
    *case, ref = _ann_case(N, B_, NH, nW, masked)
    _check_ann(lambda: _run_ann(case, NH, nW), ref, N, masked, B_, NH, f"N={N} mask={masked}")


@pytest.mark.parametrize("N,Tq,masked", CASES, ids=IDS)
def test_sew_large_window(N, Tq, masked):
    B_ = nW = 4 if masked else 1
    *case, ref, bound = _sew_case(Tq, N // Tq, B_, NH, nW, masked)
    _check_sew(lambda: _run_sew(case, Tq, N // Tq, B_, NH, nW), ref, bound, N, masked, B_, NH, f"N={N} Tq={Tq} mask={masked}")


@pytest.mark.parametrize("N", [194, 225, 450])
def test_ann_ragged_tail_with_small_logits(N):
    """The ragged shapes again with |logit| <= 5.5 (and the mask): a key past N admitted with logit 0 now carries a visible share of
    a row's weight instead of e^-14 - the select of the last block is visible (keys N.. of the last key tile: +2, +3 at 194 and 450,
    +1 .. +3 at 225; and the 14 / 62 keys of the last block's absent tiles at 194 and 450)."""
    *case, ref = _ann_case(N, 4, NH, 4, True, low=True)
    _check_ann(lambda: _run_ann(case, NH, 4), ref, N, True, 4, NH, f"N={N} low logits")


# ---------------------------------------------------------------- the window partition / reverse inside the kernel
B_W, D_W, H_W, W_W, WS, SS = 1, 4, 20, 33, (2, 15, 15), (1, 7, 7)


@functools.lru_cache(maxsize=None)
def _windowed_case():
    """fp64 through the oracle's slice table (pad + roll + window partition as one index table, -1 = padding token, which reads the
    `pad` row): gather -> ann_attention_core -> scatter of the real rows."""
    Cc, seed, N = NH * 32, 21000, WS[0] * WS[1] * WS[2]
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
    o, _ = O.ann_attention_core(win, ls.double(), bias.double(), mask.double(), NH)
    ref = torch.zeros(rows, Cc, dtype=torch.float64)
    ref[src[src >= 0]] = o[src >= 0]
    return qkv, ls, bias, mask, pad, ref, B_, src


def test_ann_windowed_forward_at_450_tokens():
    """hip.win_attn_ann_windowed's call at the (2,15,15) window with shift (1,7,7) on a (1, 4, 20, 33) map: 30 x 45 padded, so every
    window row holds padding tokens (which read pad_qkv and write nothing); row_map from hip.window_slice_map, equal to the oracle's
    table; `out` NaN beforehand: every activation row is written."""
    qkv, ls, bias, mask, pad, ref, B_, src = _windowed_case()
    N = 450
    row_map, B2 = hip.window_slice_map(B_W, D_W, H_W, W_W, WS, SS, DEV)
    assert B2 == B_ == 12 == mask.shape[0] and torch.equal(row_map.cpu().view(B_, N).long(), src)
    assert bool((src < 0).view(B_, 2, 15, 15).any(-1).any(-1).all())                     # padding tokens in every window
    run = lambda: _run_ann((qkv, ls, bias, mask), NH, B_, row_map=row_map, pad=pad, B_=B_, N=N, rows=qkv.shape[0])
    _check_ann(run, ref, N, True, B_, NH, "windowed (2,15,15) shift (1,7,7)")


def test_wrappers_run_the_same_call_and_refuse_beyond_1024():
    """hip.win_attn_ann / win_attn_sew / win_attn_ann_windowed pick sdf_win_attn_large_fwd above 192 tokens and fill the descriptor as
    this file does: bit-equal results; 1025 tokens raise SdfError with the library's E_SHAPE."""
    N, B_, nW = 194, 4, 4
    qkv, ls, bias, mask, _ = _ann_case(N, B_, NH, nW, True)
    got, _ = _run_ann((qkv, ls, bias, mask), NH, nW)
    t = _dev(qkv, ls.reshape(-1), bias, mask)
    with hip.launch_log() as log:
        out = hip.win_attn_ann(*t, NH)
    assert len(log.rows) == 1 and KERNEL in log.rows[0][0]
    assert torch.equal(out.cpu().view(B_ * N, -1), got)
    q, k, v, scale, bias, mask, _, _ = _sew_case(2, N // 2, B_, NH, nW, True)
    got, _ = _run_sew((q, k, v, scale, bias, mask), 2, N // 2, B_, NH, nW)
    t = _dev(q, k, v, scale, bias, mask)
    assert torch.equal(hip.win_attn_sew(*t, NH, 2, B_, N // 2).cpu().view(B_ * N, -1), got)
    qkv, ls, bias, mask, pad, _, B_, _ = _windowed_case()
    row_map, _ = hip.window_slice_map(B_W, D_W, H_W, W_W, WS, SS, DEV)
    got, _ = _run_ann((qkv, ls, bias, mask), NH, B_, row_map=row_map, pad=pad, B_=B_, N=450, rows=qkv.shape[0])
    t = _dev(qkv, ls.reshape(-1), bias, mask, pad)
    assert torch.equal(hip.win_attn_ann_windowed(t[0], row_map, B_, 450, t[4], t[1], t[2], t[3], NH).cpu(), got)
    with hip.launch_log() as log, pytest.raises(hip.SdfError) as e:
        hip.win_attn_ann(torch.zeros((1, 1025, 288), device=DEV), torch.ones(3, device=DEV), torch.zeros((3, 8, 8), device=DEV), None, NH)
    assert e.value.rc == hip.E_SHAPE and not log.rows
