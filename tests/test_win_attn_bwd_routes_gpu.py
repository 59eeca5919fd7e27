"""The window-attention backward on every kernel route, per element: sdf_win_attn_ann_bwd (csrc/win_attn_bwd.hip) and
sdf_win_attn_sew_bwd (csrc/win_attn_sew_bwd.hip) up to 192 tokens per window, sdf_win_attn_large_ann_bwd and
sdf_win_attn_large_sew_bwd (csrc/win_attn_large_bwd.hip) above, each called through its descriptor on buffers between guard regions
and compared with the float64 formulas of tests/win_attn_bwd_cases.py (which test_win_attn_bwd_reference_cpu.py holds against
float64 autograd).

Every case asserts
  * the launch log: exactly the expected kernels in order, each with the expected grid, block and dynamic LDS - the <= 192 ANN kernel
    with (4 NP 36 + 5 NP + 4 97) 4 bytes (above 64 KiB at N = 192, the opt-in), the d_bias kernels with runs x nH x tiles workgroups,
    runs from the split restated in win_attn_bwd_cases.py - so a case that exists for a route cannot silently run another;
  * guards: inputs, outputs and the workspace lie between guard regions that must hold their marker bit for bit; the inputs are
    unchanged; outputs and workspace start as NaN and no NaN may remain in an output (a partial read before it was written, an
    element never stored);
  * determinism: a second call gives the same bits, and so does the autograd wrapper (WinAttnAnnFunction / WinAttnSewFunction), whose
    backward must log the same launches;
  * bounds, on dq, dk, dv, d_bias and each third of d_pad SEPARATELY (one bound over dqkv lets the largest third hide the others: with
    a zero pad row the k third of d_pad exceeds 1e6, under a mask max |dv| is thousands while its scale K (Q^T dO) term is order 1):
      (a) max |err| <= tol max |ref|, tol = 2e-5 (ANN) / 1e-5 (SEW): the existing bound, now per part;
      (b) per element |err| <= kappa mag + 1e-30, mag = the sum of the absolute values of the terms the element is summed from.  The
          floor covers entries whose P underflows fp32 (e^-100 under a mask);
    d_scale gets (a) alone: its magnitude is about 1e4 to 1e5 times its value, (b) would say nothing.

kappa is not tuned on the kernels: it is 8 x the worst per-element ratio of the CPU's float32 evaluation of the same formulas over the
family's cases, rounded up to one digit (win_attn_bwd_cases.KAPPA; the CPU test asserts kappa / 8):
               dq      dk      dv      d_bias
    SEW        3e-6    2e-6    3e-6    1e-6
    ANN low    6e-7    6e-7    3e-6    1e-6        scale 1.5 on every head, |bias| <= 1
    ANN high   3e-5    7e-5    3e-4    2e-4        scale up to 100 (head 0: the clamp's value), bias up to 16: logits near 116, whose
                                                   fp32 rounding (2^-24 x 116 = 7e-6) is in every P
max mag / max |ref| is 15 - 64 for dq and dk, which is why (a) stays beside (b).

What the cases are for (win_attn_bwd_cases.py): window-major N = 1, 16, 81, 128, 192 with 3 and 10 windows (one tile with idle
waves; one real token in the last tile; no ragged tile; 12 tiles; fewer windows than the reduce kernel's eight-wide loop, and once
through it with two left over), row-mapped N = 162 and 98 with padding tokens, shift and mask, a zero pad row, 12 heads; the ragged
N again with low logits, where a key admitted past N with logit 0 weighs > 5e-4 of a row instead of e^-10; SEW (Tq, N1) from (1, 1)
to (2, 96), masked and plain; and for each of the three d_bias kernels cases with two windows per run and a shorter last run (every
other case of the suite has one window per run).  N = 450 with two windows per run runs in both modes (13 windows), and N = 200
with 12 heads and a mask.  45 cases: 21 ANN and 16 SEW per-element cases, 8 exact-zero cases.
Exact zeros (== 0, no tolerance): dO zero on one window (ANN: that window's dqkv rows), one head dim of dO zero (SEW: that dim of dv),
k or q all-zero in one window (SEW: its dq / dk).

Two perturbations, by the bounds: without the `min(B_, ...)` clamp the last run of a ragged case reads window B_ - past the end of v,
dout or qkv, i.e. the guard's NaN (d_bias becomes NaN: the NaN check), or for SEW with Tq = 2 the first window of the next time step,
a whole extra dO V^T term of the size of the element's magnitude against kappa = 1e-6.  Admitting key N in the ragged tile gives it
logit 0 (its k^ is a zero row, no bias): at low logits P of every row moves by > 5e-4 relative, so dv, dS and everything behind them
move by about 5e-4 of their magnitude against kappa <= 3e-6.

Measured on an MI355X, worst over the cases of each entry point: err / mag (bound (b)) for dq, dk, dv, d_bias with the thirds of d_pad
under their part, err / max |ref| (bound (a)) for d_scale:
                                              dq       dk       dv       d_bias   d_scale
    sdf_win_attn_sew_bwd                      2.9e-7   1.7e-7   3.3e-7   1.2e-7
    sdf_win_attn_large_sew_bwd                2.9e-7   1.8e-7   2.8e-7   8.1e-8
    sdf_win_attn_ann_bwd, low logits          5.8e-8   5.5e-8   2.6e-7   1.3e-7   5.1e-7
    sdf_win_attn_ann_bwd, high logits         2.7e-6   4.8e-6   2.1e-5   1.0e-5   1.1e-5
    sdf_win_attn_large_ann_bwd, high logits   2.4e-6   7.7e-6   2.4e-5   1.3e-5   6.4e-6
Every kernel is where the CPU's float32 evaluation is (kappa / 8), none near kappa; under bound (a) the worst part is 5.9e-6 of its
largest element (ANN, d_bias at N = 450) and 1.0e-6 (SEW, dv at N = 450 masked).  No kernel defect was found.
Run time there: the 45 cases of this file in 3.7 s together; the first (which loads the library) 1.1 s, the first row-mapped one
0.3 s, every other at most 0.05 s."""
import ctypes as C

import pytest
import torch

import win_attn_bwd_cases as BC
from routes_common import short
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _up(a, b):
    return -(-a // b)


def _ann_launches(large, B_, nH, N):
    """[(kernel, workgroups, threads, dynamic LDS bytes)] of one ANN backward call"""
    bh, NP = B_ * nH, _up(N, 16) * 16
    if not large:
        lds = (4 * NP * 36 + 5 * NP + 4 * 97) * 4
        assert N < 192 or lds > 64 << 10                       # the opt-in above 64 KiB of dynamic LDS
        return [("win_attn_ann_bwd_kernel", bh, 256, lds),
                ("win_attn_ann_bwd_reduce_kernel", _up(nH * N * N + nH + 3 * nH * 32, 256), 256, 0)]
    G, runs = _up(N, 64), BC.dbias_runs(B_, BC.dbias_tiles("large_ann", nH, N))
    return [("win_attn_large_ann_bwd_query_kernel", bh * G, 256, 0), ("win_attn_large_ann_bwd_key_kernel", bh * G, 256, 0),
            ("win_attn_large_ann_bwd_dbias_kernel", runs * nH * G * G, 256, 0),
            ("win_attn_large_bwd_sum_runs_kernel", _up(nH * N * N, 256), 256, 0),
            ("win_attn_large_ann_bwd_reduce_kernel", _up(nH + 3 * nH * 32, 256), 256, 0)]


def _sew_launches(large, B_, nH, N):
    bh = B_ * nH
    if not large:
        lds = 3 * N * 32 + (((N * 33 + 3) & ~3) + 2 * 32 * 36 + N * 33) * 4
        runs = BC.dbias_runs(B_, BC.dbias_tiles("sew", nH, N))
        return [("sew_bwd_kernel", bh, 256, lds), ("sew_bwd_dbias_kernel", runs * nH * _up(N, 16), _up(N, 64) * 64, 0),
                ("sew_bwd_dbias_finish_kernel", _up(nH * N * N, 256), 256, 0)]
    runs = BC.dbias_runs(B_, BC.dbias_tiles("large_sew", nH, N))
    return [("win_attn_large_sew_bwd_gram_kernel", bh, 256, 0), ("win_attn_large_sew_bwd_dv_kernel", bh * _up(N, 64), 256, 0),
            ("win_attn_large_sew_dbias_kernel", runs * nH * _up(N, 16) * _up(N, 256), 256, 0),
            ("win_attn_large_bwd_sum_runs_kernel", _up(nH * N * N, 256), 256, 0)]


def _attn_rows(log):
    return [(short(k), wgs, thr, lds) for k, wgs, thr, lds, _ in log.rows if "win_attn" in k or "sew_bwd" in k]


def _guarded_call(entry, desc, ins, outs, B_, nH, N, fill):
    """One call of `entry` with every buffer between guard regions -> ({output name: tensor}, launch rows).  ins: name -> device
    tensor; outs: name -> shape (fp32); fill(d, ptr) sets the desc's fields from ptr(name) (None for an absent input)."""
    gi = {k: BC.guarded(tuple(v.shape), v.dtype, DEV, v) for k, v in ins.items()}
    nbytes = getattr(hip.lib(), entry + "_workspace_bytes")(B_, nH, N)
    assert nbytes > 0 and nbytes % 256 == 0
    go = {k: BC.guarded(shape, torch.float32, DEV) for k, shape in outs.items()}
    go["ws"] = BC.guarded((nbytes // 4,), torch.float32, DEV)

    def ptr(k):
        t = gi.get(k) or go.get(k)
        return t[1].data_ptr() if t else None
    d = desc()
    fill(d, ptr)
    d.workspace, d.workspace_bytes = go["ws"][1].data_ptr(), nbytes
    with hip.launch_log() as log:
        rc = getattr(hip.lib(), entry)(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, (buf, mid) in gi.items():
        BC.guards_hold(buf, "input " + k)
        assert torch.equal(mid, ins[k]), f"input {k} was written"
    for k, (buf, mid) in go.items():
        BC.guards_hold(buf, "output " + k)
        if k != "ws":
            assert not torch.isnan(mid).any(), f"output {k}: an element was never written, or a NaN was read"
    return {k: go[k][1] for k in outs}, _attn_rows(log)


def _ann_call(large, x):
    entry = "sdf_win_attn_large_ann_bwd" if large else "sdf_win_attn_ann_bwd"
    B_, nH, N = x["B_"], x["nH"], x["N"]
    ins = {k: x[k] for k in ("qkv", "pad", "ls", "bias", "dout", "row_map", "mask") if x[k] is not None}
    outs = {"dqkv": tuple(x["qkv"].shape), "d_pad": tuple(x["pad"].shape), "d_scale": (nH,), "d_bias": (nH, N, N)}

    def fill(d, p):
        d.qkv, d.row_map, d.pad_qkv, d.dout = p("qkv"), p("row_map"), p("pad"), p("dout")
        d.scale, d.bias, d.mask = p("ls"), p("bias"), p("mask")
        d.dqkv, d.d_pad, d.d_scale, d.d_bias = p("dqkv"), p("d_pad"), p("d_scale"), p("d_bias")
        d.B_, d.nW, d.nH, d.N, d.hd = B_, (x["mask"].shape[0] if x["mask"] is not None else 1), nH, N, 32
    return _guarded_call(entry, hip.WinAttnBwdDesc, ins, outs, B_, nH, N, fill)


def _sew_call(large, x):
    entry = "sdf_win_attn_large_sew_bwd" if large else "sdf_win_attn_sew_bwd"
    Tq, B_, N1, Cc = x["q"].shape
    nH, N = x["nH"], Tq * N1
    ins = {k: x[k] for k in ("q", "k", "v", "sc", "bias", "dout", "mask") if x[k] is not None}
    outs = {"dq": (Tq, B_, N1, Cc), "dk": (Tq, B_, N1, Cc), "dv": (Tq, B_, N1, Cc), "d_bias": (nH, N, N)}

    def fill(d, p):
        d.q, d.k, d.v, d.dout, d.scale, d.bias, d.mask = p("q"), p("k"), p("v"), p("dout"), p("sc"), p("bias"), p("mask")
        d.dq, d.dk, d.dv, d.d_bias = p("dq"), p("dk"), p("dv"), p("d_bias")
        d.B_, d.nW, d.nH, d.Tq, d.N1, d.hd = B_, (x["mask"].shape[0] if x["mask"] is not None else 1), nH, Tq, N1, 32
    return _guarded_call(entry, hip.WinAttnSewBwdDesc, ins, outs, B_, nH, N, fill)


def _bounds(tag, mode, family, got, ref, mag):
    """bounds (a) and (b) on every part; prints each figure before it asserts"""
    bad = []
    for part in ref:
        err = (got[part].double() - ref[part]).abs().max().item()
        top = ref[part].abs().max().item()
        ratio, kappa = BC.worst_ratio(got[part], ref[part], mag[part]), BC.kappa_of(family, part)
        print(f"WINATTN-BWD {tag} {part}: (a) {err:.3e} = {err / top if top else 0.0:.2e} of max |ref| {top:.3e}   "
              f"(b) worst err / mag {ratio:.2e}, kappa {kappa:.0e}")
        if not err <= BC.TOL[mode] * top:
            bad.append((part, "a", err, top))
        if not ratio <= kappa:
            bad.append((part, "b", ratio, kappa))
    assert not bad, bad


def _ann_device(name):
    x = BC.cast(BC.ann_inputs(name), torch.float32, DEV)
    return {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in x.items()}


ANN_PARAMS = [(n, False) for n in BC.ANN_CASES] + [(n, True) for n in BC.ANN_LARGE_CASES]


@pytest.mark.parametrize("name,large", ANN_PARAMS)
def test_ann_backward_per_element(name, large):
    from sdformerflow_amd.autograd import WinAttnAnnFunction
    c = {**BC.ANN_CASES, **BC.ANN_LARGE_CASES}[name]
    x = _ann_device(name)
    B_, nH, N = x["B_"], x["nH"], x["N"]
    assert large == (N > 192)
    out, rows = _ann_call(large, x)
    assert rows == _ann_launches(large, B_, nH, N), rows
    again, _ = _ann_call(large, x)
    assert all(torch.equal(out[k], again[k]) for k in out), "two calls differ"

    leaf = {k: x[k].clone().requires_grad_(True) for k in ("qkv", "ls", "bias", "pad")}
    o = WinAttnAnnFunction.apply(leaf["qkv"], leaf["ls"], leaf["bias"], leaf["pad"], x["row_map"], B_, N, x["mask"], nH)
    with hip.launch_log() as log:
        (o * x["dout"]).sum().backward()
    torch.cuda.synchronize()
    assert _attn_rows(log) == rows, _attn_rows(log)
    for k, g in (("dqkv", "qkv"), ("d_pad", "pad"), ("d_scale", "ls"), ("d_bias", "bias")):
        assert torch.equal(leaf[g].grad, out[k]), f"the autograd wrapper's {k} differs"

    x64 = BC.cast(x, torch.float64)
    ref, mag = BC.ann_eval(x64), BC.ann_eval(x64, absolute=True)
    tag = f"{'large_ann' if large else 'ann'} {name}"
    err, top = (out["d_scale"].double() - ref[2]).abs().max().item(), ref[2].abs().max().item()
    print(f"\nWINATTN-BWD {tag} d_scale: (a) {err:.3e} = {err / top if top else 0.0:.2e} of max |ref| {top:.3e}")
    _bounds(tag, "ann", BC.ann_family(c), BC.ann_parts(out["dqkv"], out["d_pad"], out["d_bias"]),
            BC.ann_parts(ref[0], ref[1], ref[3]), BC.ann_parts(mag[0], mag[1], mag[3]))
    assert err <= BC.TOL["ann"] * top, ("d_scale", err, top)
    if c["kind"] == "wm":
        assert not out["d_pad"].any()                           # no padding token without a row map
    if c["zero_pad"]:                                           # k of a padding token is 0: the normalize eps carries its gradient
        assert ref[1][nH * 32:2 * nH * 32].abs().max().item() > 1e6


def _sew_device(name):
    inp = BC.sew_inputs(name)
    x = BC.cast(inp, torch.float32, DEV)
    for t in "qkv":
        x[t] = x[t].to(torch.uint8).contiguous()
    x["sc"] = torch.full((inp["nH"],), inp["scale"], device=DEV)
    assert float(x["sc"][0]) == inp["scale"]
    return x


SEW_PARAMS = [(n, False) for n in BC.SEW_CASES] + [(n, True) for n in BC.SEW_LARGE_CASES]


@pytest.mark.parametrize("name,large", SEW_PARAMS)
def test_sew_backward_per_element(name, large):
    from sdformerflow_amd.autograd import WinAttnSewFunction
    x = _sew_device(name)
    Tq, B_, N1, _ = x["q"].shape
    nH, N = x["nH"], Tq * N1
    assert large == (N > 192)
    out, rows = _sew_call(large, x)
    assert rows == _sew_launches(large, B_, nH, N), rows
    again, _ = _sew_call(large, x)
    assert all(torch.equal(out[k], again[k]) for k in out), "two calls differ"

    leaf = {k: x[k].float().clone().requires_grad_(True) for k in ("q", "k", "v", "bias")}
    o = WinAttnSewFunction.apply(leaf["q"], leaf["k"], leaf["v"], leaf["bias"], x["sc"], x["mask"], nH)
    with hip.launch_log() as log:
        (o * x["dout"]).sum().backward()
    torch.cuda.synchronize()
    assert _attn_rows(log) == rows, _attn_rows(log)
    for k, g in (("dq", "q"), ("dk", "k"), ("dv", "v"), ("d_bias", "bias")):
        assert torch.equal(leaf[g].grad, out[k]), f"the autograd wrapper's {k} differs"

    x64 = BC.cast(BC.sew_inputs(name), torch.float64, DEV)
    names = ("dq", "dk", "dv", "d_bias")
    ref, mag = dict(zip(names, BC.sew_eval(x64))), dict(zip(names, BC.sew_eval(x64, absolute=True)))
    print()
    _bounds(f"{'large_sew' if large else 'sew'} {name}", "sew", "sew", out, ref, mag)


# ---------------------------------------------------------------------------------------------------------------------- exact zeros
@pytest.mark.parametrize("name,large", [("wm81_b3_mask", False), ("wm200_b51_mask", True)])
def test_ann_window_without_dout_gets_exactly_zero(name, large):
    """dO = 0 on one whole window: dP, D and dS of the window are 0, so its dq, dk and dv rows are exactly 0 - anything else leaked in
    from another window."""
    x = _ann_device(name)
    B_, N = x["B_"], x["N"]
    dout = x["dout"].clone()
    dout.view(B_, N, -1)[1] = 0
    bwd = hip.win_attn_ann_bwd_large if large else hip.win_attn_ann_bwd
    dqkv, _, _, _ = bwd(x["qkv"], None, B_, N, x["pad"], x["ls"], x["bias"], x["mask"], x["nH"], dout)
    torch.cuda.synchronize()
    assert bool((dqkv.view(B_, N, -1)[1] == 0).all())
    assert bool(dqkv.view(B_, N, -1)[0].any()) and bool(dqkv.view(B_, N, -1)[2].any())


@pytest.mark.parametrize("name,large", [("w2x81_mask", False), ("w1x193_b59", True)])
@pytest.mark.parametrize("what", ["dout_dim", "k_window", "q_window"])
def test_sew_exact_zeros(name, large, what):
    """One head dim of dO zero: that dim of dv is exactly 0 (every term of it carries that dim of dO).  k all-zero in one window:
    V^T K = 0, its dq is exactly 0; q all-zero in one window: Q^T dO = 0, its dk is exactly 0."""
    x = _sew_device(name)
    Tq, B_, N1, _ = x["q"].shape
    nH = x["nH"]
    q, k, dout = x["q"].clone(), x["k"].clone(), x["dout"].clone()
    if what == "dout_dim":
        dout.view(Tq, B_, N1, nH, 32)[..., 5] = 0
    elif what == "k_window":
        k.view(B_, nH, Tq * N1, 32)[1] = 0                      # the raw head view: window 1 is one contiguous block
    else:
        q.view(B_, nH, Tq * N1, 32)[1] = 0
    bwd = hip.win_attn_sew_bwd_large if large else hip.win_attn_sew_bwd
    dq, dk, dv = (t.view(B_, nH, Tq * N1, 32) for t in bwd(q, k, x["v"], x["sc"], x["bias"], x["mask"], nH, Tq, B_, N1, dout)[:3])
    torch.cuda.synchronize()
    if what == "dout_dim":
        assert bool((dv[..., 5] == 0).all()) and bool(dv[..., 4].any())
    elif what == "k_window":
        assert bool((dq[1] == 0).all()) and bool(dq[0].any())
    else:
        assert bool((dk[1] == 0).all()) and bool(dk[0].any())
