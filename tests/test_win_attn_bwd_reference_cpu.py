"""What tests/test_win_attn_bwd_routes_gpu.py measures the window-attention backward kernels against, checked without a GPU
(tests/win_attn_bwd_cases.py):

  * the backward written out as formulas in float64 equals float64 autograd - through the oracle's `sew_attention_core`, and for the
    ANN through the materialised composition (pad with the pad row, roll, window partition, the oracle's `ann_attention_core`, window
    reverse, roll back, crop) - to 1e-12 of each tensor's largest element (measured: 7e-15 at most);
  * the same formulas evaluated in float32 stay within kappa / 8 of the float64 result per element, in units of the element's
    magnitude: the constants of the GPU file's bound (b) come from here and not from the kernels.  Every case prints its ratios;
    win_attn_bwd_cases.KAPPA records the worst per family and part;
  * the d_bias run split of the three kernels that have one, restated: every case that exists for the in-workgroup window loop has
    at least two windows per run, and those that exist for the ragged last run have a shorter last run."""
import pytest
import torch
import torch.nn.functional as F

import win_attn_bwd_cases as BC
from oracle import sdformer_oracle as O
from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw

ANN_ALL = {**BC.ANN_CASES, **BC.ANN_LARGE_CASES}
SEW_ALL = {**BC.SEW_CASES, **BC.SEW_LARGE_CASES}


def _same(got, ref, what):
    err, top = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"    {what}: max |formula - autograd| {err:.3e}, max |autograd| {top:.3e}")
    assert err <= 1e-12 * top, (what, err, top)


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("name", ["w1x1", "w1x45_mask", "w1x65", "w2x81_mask", "w2x96_mask", "w1x193_b59"])
def test_sew_formulas_equal_fp64_autograd(name):
    inp = BC.cast(BC.sew_inputs(name), torch.float64)
    Tq, B_, N1, _ = inp["q"].shape
    nH = inp["nH"]
    r = [_leaf(inp[t].reshape(B_, nH, Tq * N1, BC.HD)) for t in "qkv"]
    rb = _leaf(inp["bias"])
    z, _ = O.sew_attention_core(r[0], r[1], r[2], inp["scale"], rb, inp["mask"], Tq, N1)
    (z * inp["dout"]).sum().backward()
    got = BC.sew_eval(inp)
    print(f"sew {name}:")
    for what, g, a in zip(("dq", "dk", "dv"), got, r):
        _same(g, a.grad.reshape(g.shape), what)
    _same(got[3], rb.grad, "d_bias")


@pytest.mark.parametrize("name", ["wm1_b3_mask", "wm16_b10", "wm81_b3_mask_low", "wm192_b3_mask", "rm162_shift", "rm98_shift_low",
                                  "rm162_zero_pad"])
def test_ann_formulas_equal_fp64_autograd(name):
    c = ANN_ALL[name]
    inp = BC.cast(BC.ann_inputs(name), torch.float64)
    nH, B_, N = inp["nH"], inp["B_"], inp["N"]
    qkv, pad, ls, bias = (_leaf(inp[t]) for t in ("qkv", "pad", "ls", "bias"))
    if c["kind"] == "wm":
        o, _ = O.ann_attention_core(qkv.view(B_, N, -1), ls.view(nH, 1, 1), bias, inp["mask"], nH)
        o = o.reshape(B_ * N, -1)
    else:
        (B, D, H, W), ws = c["grid"], c["ws"]
        ss = tuple(w // 2 for w in ws) if c["shifted"] else (0, 0, 0)
        Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
        grow = (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D)
        real = F.pad(torch.ones((B, D, H, W, 1), dtype=qkv.dtype), grow) > 0
        x = torch.where(real, F.pad(qkv.view(B, D, H, W, -1), grow), pad)
        x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
        o, _ = O.ann_attention_core(sw.window_partition(x, ws), ls.view(nH, 1, 1), bias, inp["mask"], nH)
        o = torch.roll(sw.window_reverse(o, ws, B, Dp, Hp, Wp), shifts=ss, dims=(1, 2, 3))[:, :D, :H, :W].reshape(B * D * H * W, -1)
    (o * inp["dout"]).sum().backward()
    got = BC.ann_eval(inp)
    print(f"ann {name}:")
    for what, g, a in zip(("dqkv", "d_pad", "d_scale", "d_bias"), got, (qkv, pad, ls, bias)):
        if what == "d_pad" and c["kind"] == "wm":
            assert not g.any() and (a.grad is None or not a.grad.any())
            continue
        _same(g, a.grad, what)
    if c["zero_pad"]:                                           # k of a padding token is 0: the normalize eps carries its gradient
        Cc = nH * BC.HD
        assert got[1][Cc:2 * Cc].abs().max().item() > 1e6


def _fp32_ratios(family, parts32, parts64, mags):
    worst = {}
    for part in parts64:
        r = BC.worst_ratio(parts32[part], parts64[part], mags[part])
        key = part.split(".")[-1]
        worst[key] = max(worst.get(key, 0.0), r)
        print(f"    {part}: worst |fp32 - fp64| / magnitude {r:.2e}   kappa / 8 = {BC.kappa_of(family, part) / 8:.2e}")
        assert r <= BC.kappa_of(family, part) / 8, (part, r)
    return worst


@pytest.mark.parametrize("name", list(SEW_ALL))
def test_sew_fp32_evaluation_is_within_an_eighth_of_kappa(name):
    inp = BC.sew_inputs(name)
    ref, mag, f32 = BC.sew_eval(BC.cast(inp, torch.float64)), BC.sew_eval(BC.cast(inp, torch.float64), absolute=True), BC.sew_eval(inp)
    names = ("dq", "dk", "dv", "d_bias")
    print(f"sew {name}:")
    _fp32_ratios("sew", dict(zip(names, f32)), dict(zip(names, ref)), dict(zip(names, mag)))


@pytest.mark.parametrize("name", list(ANN_ALL))
def test_ann_fp32_evaluation_is_within_an_eighth_of_kappa(name):
    inp = BC.ann_inputs(name)
    ref, mag, f32 = BC.ann_eval(BC.cast(inp, torch.float64)), BC.ann_eval(BC.cast(inp, torch.float64), absolute=True), BC.ann_eval(inp)
    print(f"ann {name} ({BC.ann_family(ANN_ALL[name])}):")
    _fp32_ratios(BC.ann_family(ANN_ALL[name]), *(BC.ann_parts(t[0], t[1], t[3]) for t in (f32, ref, mag)))
    # d_scale: its magnitude is thousands of times its value, so bound (b) says nothing and the GPU file keeps bound (a) alone for it
    err, top = (f32[2].double() - ref[2]).abs().max().item(), ref[2].abs().max().item()
    if top:                                                     # (a one-token window has dS = 0)
        print(f"    d_scale: {err / top:.2e} of max |ref|, magnitude / |ref| up to {(mag[2] / ref[2].abs()).max().item():.1e}")


def test_the_runs_cases_reach_the_window_loop_and_the_ragged_last_run():
    assert set(BC.RUNS_CASES) <= set(ANN_ALL) | set(SEW_ALL) and set(BC.RAGGED_LAST_RUN) <= set(BC.RUNS_CASES)
    for name, (kernel, B_, nH, N) in BC.RUNS_CASES.items():
        if name in ANN_ALL:
            assert (ANN_ALL[name]["B_"], ANN_ALL[name]["nH"], ANN_ALL[name]["N"]) == (B_, nH, N)
        else:
            Tq, N1, b, _, h = SEW_ALL[name]
            assert (b, h, Tq * N1) == (B_, nH, N)
        assert (kernel == "sew") == (N <= 192)
        tiles = BC.dbias_tiles(kernel, nH, N)
        wrun, runs = BC.dbias_run(B_, tiles), BC.dbias_runs(B_, tiles)
        assert wrun >= 2 and (runs - 1) * wrun < B_ <= runs * wrun, (name, wrun, runs)
        if name in BC.RAGGED_LAST_RUN:
            assert B_ - (runs - 1) * wrun < wrun, (name, wrun, runs)
    # the figures the case table quotes
    assert (BC.dbias_run(23, 144), BC.dbias_runs(23, 144)) == (2, 12) and (BC.dbias_run(101, 33), BC.dbias_runs(101, 33)) == (2, 51)
    assert (BC.dbias_run(50, 48), BC.dbias_runs(50, 48)) == (2, 25) and (BC.dbias_run(51, 48), BC.dbias_runs(51, 48)) == (2, 26)
    assert (BC.dbias_run(59, 39), BC.dbias_runs(59, 39)) == (2, 30)
    # ... and every other case of the existing files has one window per run
    assert BC.dbias_run(12, 3 * 11) == 1 and BC.dbias_run(4, BC.dbias_tiles("large_ann", 3, 200)) == 1
