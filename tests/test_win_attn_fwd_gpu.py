"""Forward of the fused window attention (csrc/win_attn.hip, sdf_win_attn_fwd) on every kernel route, against the oracle's matrix
cores (oracle.sdformer_oracle.ann_attention_core / sew_attention_core) evaluated in float64 on the same fp32 / byte inputs.

Three kernels sit behind the one entry point: the fp16-split matrix-pipe kernel win_attn_tiled_f16_kernel (the default for even N
with 8 or 11 key tiles), the exact-fp32 tiled kernel win_attn_tiled_kernel (SDF_ATTN_F32=1, or an output beyond 2^31 bytes) and the
general kernel win_attn_kernel (odd N, any other tile count, SDF_ATTN_GENERIC=1).  Every case here

  * asserts through hip.launch_log() that exactly ONE launch happened and that it was the expected kernel, with the expected mode,
    tile count and mask flag in its template arguments - a parity test that silently ran another kernel proves nothing;
  * hands the kernel an `out` that is a slice of a larger buffer, 64 guard rows on each side, everything NaN beforehand: the guards
    must still hold the same NaN bits, no NaN may remain inside (the fp16 kernel stores through a 2^31-1 byte buffer descriptor,
    nothing clamps a wrong row there);
  * runs the call twice: bit-equal results.

Bounds.  ANN (cosine softmax, |v| <= 1): max |got - ref64| <= 2e-5, the project's bound; the fp32 evaluation of the reference itself
is up to 8.3e-6 from fp64 for these inputs (logits up to 100 + 16, exp amplifies their fp32 rounding), which is why the comparison
is with fp64.  SEW (spiking, no softmax): per element |got - ref64| <= 1e-5 * (|attn64| @ v), through the same output scramble as the
result, and exact equality where that sum is 0: three fp32 roundings of a score, 22 bits of the fp16 split and fp32 accumulation over
N <= 192 terms stay below 4e-6 of the absolute sum.  (A bound relative to max |ref| would let 0.04 through under a -100 mask.)

The recipe's logits are large (bias up to 14, logit scale up to 100), so a key wrongly admitted past the ragged tail with logit 0
would weigh e^-14 and pass; the `low` cases repeat the ragged shapes with |logit| <= 5.5, where such a key weighs > 2e-4.

Largest error measured on an MI355X (all cases of this file):
  ANN, max |got - ref64|:         win_attn_tiled_f16_kernel 7.7e-6   win_attn_tiled_kernel 9.9e-6   win_attn_kernel 9.9e-6
  SEW, max |err| / (|attn| @ v):  win_attn_tiled_f16_kernel 5.7e-7   win_attn_tiled_kernel 8.4e-7   win_attn_kernel 8.4e-7
Run time there: the 104 cases of this file in 3.1 s together; the slowest (the first, which loads the library) 0.4 s, every other
below 0.15 s."""
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
ROUTES = {"default": None, "f32": "SDF_ATTN_F32", "generic": "SDF_ATTN_GENERIC"}
F16, F32, GEN = "win_attn_tiled_f16_kernel", "win_attn_tiled_kernel", "win_attn_kernel"


def _expected_kernel(route, N):
    nt = (N + 15) // 16
    if route == "generic" or N % 2 or nt not in (8, 11):
        return GEN
    return F32 if route == "f32" else F16


def _assert_one_launch(log, kernel, mode, N, masked, B_, nH):
    """Exactly one launch, of `kernel`<mode[, tiles, mask]>, one workgroup of 256 threads per (window, head)."""
    assert len(log.rows) == 1, log.rows
    name, wgs, threads, lds, _ = log.rows[0]
    nt, m = (N + 15) // 16, int(mode == "sew")
    if kernel == GEN:
        want = (f"{GEN}<{m}>", f"{GEN}ILi{m}EE")
    else:
        want = (f"{kernel}<{m}, {nt}, {'true' if masked else 'false'}>", f"{kernel}ILi{m}ELi{nt}ELb{int(masked)}EE")
    assert want["<" not in name] in name, (name, want)           # demangled, or the mangled name when the demangler gave up
    assert wgs == B_ * nH and threads == 256
    if kernel == GEN and nt == 12:
        assert lds == 3 * 192 * 36 * 4 > 64 << 10                # the opt-in above 64 KiB of dynamic LDS
    return name


def _switch(monkeypatch, route):
    for name in ("SDF_ATTN_F32", "SDF_ATTN_GENERIC"):
        monkeypatch.delenv(name, raising=False)
    if ROUTES[route]:
        monkeypatch.setenv(ROUTES[route], "1")


def _mask(N, nW, seed):
    """(nW, N, N) 0 / -100: the shifted-window mask of the two real windows, else from random labels in {0, 1, 2} per window
    (-100 where the labels differ: the diagonal is 0, no row is fully masked)."""
    if (N, nW) == (128, 4):
        return O.compute_mask(2, 16, 16, (2, 8, 8), (1, 4, 4))
    if (N, nW) == (162, 4):
        return O.compute_mask(2, 18, 18, (2, 9, 9), (1, 4, 4))
    lab = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).integers(0, 3, (nW, N)))
    return torch.where(lab[:, :, None] != lab[:, None, :], torch.tensor(-100.0), torch.tensor(0.0))


def _ann_params(nH, N, seed, low=False):
    """(logit_scale (nH,1,1), bias (nH,N,N)): the recipe of test_hip_kernels.test_win_attn_ann_cosine_softmax with head 0 at exactly
    100 (the largest logits carry the largest error); low: |logit| <= e^1.5 + 1."""
    if low:
        return torch.full((nH, 1, 1), math.exp(1.5)), rnd((nH, N, N), seed + 2, -1.0, 1.0)
    ls = torch.exp(torch.clamp(rnd((nH, 1, 1), seed + 1, 1.5, 5.0), max=math.log(100.0)))
    ls[0] = 100.0
    return ls, 16 * torch.sigmoid(rnd((nH, N, N), seed + 2, -2.0, 2.0))


@functools.lru_cache(maxsize=None)
def _ann_case(N, B_, nH, nW, masked, low=False):
    """Inputs and the fp64 reference of one ANN case, shared by the routes that run it."""
    seed = 7000 + 16 * N + int(masked) + 2 * int(low)
    qkv = rnd((B_, N, 3 * nH * 32), seed, -1.0, 1.0)
    ls, bias = _ann_params(nH, N, seed, low)
    mask = _mask(N, nW, seed + 3) if masked else None
    ref, _ = O.ann_attention_core(qkv.double(), ls.double(), bias.double(), mask.double() if masked else None, nH)
    return qkv, ls, bias, mask, ref.reshape(B_ * N, nH * 32)


@functools.lru_cache(maxsize=None)
def _sew_case(Tq, N1, B_, nH, nW, masked):
    """Inputs, the fp64 reference and the per-element bound 1e-5 * (|attn64| @ v) of one SEW case."""
    N, Cc = Tq * N1, nH * 32
    seed = 9000 + 16 * N + int(masked)
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
    """One sdf_win_attn_fwd call into a NaN-filled, guarded `out` -> (result (rows, Cc) on the CPU, launch log).  `fill(d)` sets
    everything but `out` (and holds the device tensors)."""
    buf = torch.full((GUARD + rows + GUARD, Cc), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    nan_bits = int(bits[0, 0])
    d = hip.WinAttnDesc()
    fill(d)
    d.out = buf[GUARD:].data_ptr()
    with hip.launch_log() as log:
        rc = hip.lib().sdf_win_attn_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
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


def _check_ann(run, ref, kernel, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, kernel, "ann", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an output row was never written"
    err = (got.double() - ref).abs().max().item()
    print(f"\nWINATTN ann {kernel} {what} err {err:.3e}  [{name}]")
    assert err <= ANN_TOL, err
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"


def _check_sew(run, ref, bound, kernel, N, masked, B_, nH, what):
    got, log = run()
    name = _assert_one_launch(log, kernel, "sew", N, masked, B_, nH)
    assert not torch.isnan(got).any(), "an output row was never written"
    err = (got.double() - ref).abs()
    zero = bound == 0
    rel = (err[~zero] / bound[~zero]).max().item() * SEW_TOL
    print(f"\nWINATTN sew {kernel} {what} err/(|attn|@v) {rel:.3e}  [{name}]")
    assert bool(zero.view(-1, 32)[:, 5].all()) and torch.equal(got[zero].double(), ref[zero]), "an element whose every term is 0 is not exactly 0"
    assert bool((err <= bound).all()), rel
    again, _ = run()
    assert torch.equal(got, again), "two calls differ"


# N: (B_, nH, nW) - between them B_ * nH = 24 with two batch copies per mask window, 12 (8 workgroup ids remapped over the XCDs, 4 not),
# 6 (fewer than one id per XCD) and a case with 6 heads
TILED = {128: (8, 3, 4), 114: (4, 3, 4), 126: (2, 3, 2), 162: (8, 3, 4), 176: (4, 6, 4)}
GENERAL = {98: (4, 3, 2), 75: (2, 3, 2), 17: (4, 3, 4), 192: (2, 3, 2), 190: (2, 6, 2)}


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N", list(TILED))
@pytest.mark.parametrize("route", list(ROUTES))
def test_ann_route_matrix(monkeypatch, route, N, masked):
    """8 tiles whole (128, the (2,8,8) window), with a 2-key tail (114), with a tail of which only one 8-byte half of a lane group's
    strip is in range (126); 11 tiles with a 2-key tail (162, the (2,9,9) window) and whole (176) - on each of the three kernels."""
    B_, nH, nW = TILED[N]
    _switch(monkeypatch, route)
    *case, ref = _ann_case(N, B_, nH, nW, masked)
    _check_ann(lambda: _run_ann(case, nH, nW), ref, _expected_kernel(route, N), N, masked, B_, nH, f"{route} N={N} mask={masked}")


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N", list(TILED))
@pytest.mark.parametrize("route", list(ROUTES))
def test_sew_route_matrix(monkeypatch, route, N, masked):
    B_, nH, nW = TILED[N]
    Tq, N1 = 2, N // 2
    _switch(monkeypatch, route)
    *case, ref, bound = _sew_case(Tq, N1, B_, nH, nW, masked)
    _check_sew(lambda: _run_sew(case, Tq, N1, B_, nH, nW), ref, bound, _expected_kernel(route, N), N, masked, B_, nH,
               f"{route} N={N} mask={masked}")


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N", list(GENERAL))
def test_ann_general_kernel_without_a_switch(monkeypatch, N, masked):
    """What takes the general kernel by itself: 7 tiles (98, the (2,7,7) window), odd N (75), one token in the second tile (17), and
    the two sizes whose 3 x 192 x 36 floats of LDS need the opt-in above 64 KiB (192 whole, 190 with a 2-key tail)."""
    B_, nH, nW = GENERAL[N]
    _switch(monkeypatch, "default")
    *case, ref = _ann_case(N, B_, nH, nW, masked)
    _check_ann(lambda: _run_ann(case, nH, nW), ref, GEN, N, masked, B_, nH, f"general N={N} mask={masked}")


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("N,Tq", [(98, 2), (75, 3), (192, 2), (190, 2)])
def test_sew_general_kernel_without_a_switch(monkeypatch, N, Tq, masked):
    B_, nH, nW = GENERAL[N]
    _switch(monkeypatch, "default")
    *case, ref, bound = _sew_case(Tq, N // Tq, B_, nH, nW, masked)
    _check_sew(lambda: _run_sew(case, Tq, N // Tq, B_, nH, nW), ref, bound, GEN, N, masked, B_, nH, f"general N={N} mask={masked}")


@pytest.mark.parametrize("route,N", [(r, n) for r in ROUTES for n in (114, 126)] + [("default", n) for n in (17, 75, 190)])
def test_ann_ragged_tail_with_small_logits(monkeypatch, route, N):
    """The ragged shapes again with |logit| <= 5.5 (and the mask): a key past N admitted with logit 0 now carries more than 2e-4 of a
    row's weight instead of e^-14 - every last-tile select is visible (keys N.. of the last tile: +2, +3 at 114 / 126 / 190, +1 at
    17, +3 at 75)."""
    B_, nH, nW = {**TILED, **GENERAL}[N]
    _switch(monkeypatch, route)
    *case, ref = _ann_case(N, B_, nH, nW, True, low=True)
    _check_ann(lambda: _run_ann(case, nH, nW), ref, _expected_kernel(route, N), N, True, B_, nH, f"{route} N={N} low logits")


# ---------------------------------------------------------------- the window partition / reverse inside the kernel
def _partition(x, ws):
    B, D, H, W, Cc = x.shape
    x = x.reshape(B, D // ws[0], ws[0], H // ws[1], ws[1], W // ws[2], ws[2], Cc)
    return x.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(-1, ws[0] * ws[1] * ws[2], Cc)


def _reverse(win, ws, B, D, H, W):
    x = win.reshape(B, D // ws[0], H // ws[1], W // ws[2], ws[0], ws[1], ws[2], -1)
    return x.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D, H, W, -1)


WINDOWED = {                 # name: (B, ws, shift, zero pad row); D, H, W = 2, 11, 20: padding tokens in H and in W
    "w9": (1, (2, 9, 9), (0, 0, 0), False),
    "w9_shift": (1, (2, 9, 9), (1, 4, 4), False),
    "w8_shift": (1, (2, 8, 8), (1, 4, 4), False),
    "w7_shift": (1, (2, 7, 7), (1, 3, 3), False),
    "w9_shift_zero_pad": (1, (2, 9, 9), (1, 4, 4), True),
    "w8_shift_two_samples": (2, (2, 8, 8), (1, 4, 4), False),
}
D_, H_, W_, NH_ = 2, 11, 20, 3


@functools.lru_cache(maxsize=None)
def _windowed_case(name):
    """fp64, materialised: pad (padding tokens read the `pad` row) -> roll -> window_partition -> ann_attention_core ->
    window_reverse -> roll back -> crop."""
    B, ws, ss, zero_pad = WINDOWED[name]
    Cc, seed = NH_ * 32, 11000 + 10 * list(WINDOWED).index(name)
    rows = B * D_ * H_ * W_
    qkv = rnd((rows, 3 * Cc), seed, -1.0, 1.0)
    pad = torch.zeros(3 * Cc) if zero_pad else rnd((3 * Cc,), seed + 4, -1.0, 1.0)
    N = ws[0] * ws[1] * ws[2]
    ls, bias = _ann_params(NH_, N, seed)
    Dp, Hp, Wp = D_ + (-D_) % ws[0], H_ + (-H_) % ws[1], W_ + (-W_) % ws[2]
    mask = O.compute_mask(Dp, Hp, Wp, ws, ss) if any(ss) else None
    x = pad.double().expand(B, Dp, Hp, Wp, 3 * Cc).clone()
    x[:, :D_, :H_, :W_] = qkv.double().view(B, D_, H_, W_, 3 * Cc)
    x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    o, _ = O.ann_attention_core(_partition(x, ws), ls.double(), bias.double(), mask.double() if mask is not None else None, NH_)
    o = torch.roll(_reverse(o, ws, B, Dp, Hp, Wp), shifts=ss, dims=(1, 2, 3))
    return qkv, ls, bias, mask, pad, o[:, :D_, :H_, :W_].reshape(rows, Cc)


@pytest.mark.parametrize("name,route", [(n, r) for n in WINDOWED for r in ROUTES if r == "default" or "w7" not in n])
def test_ann_windowed_forward(monkeypatch, name, route):
    """hip.win_attn_ann_windowed's call - row_map from hip.window_slice_map, padding tokens reading pad_qkv - against the materialised
    reference; `out` NaN beforehand: every activation row is written (the wrapper's torch.zeros would hide one that is not).  A zero
    pad row makes the padding tokens' k the zero vector: F.normalize's eps decides their cosine."""
    B, ws, ss, _ = WINDOWED[name]
    N = ws[0] * ws[1] * ws[2]
    _switch(monkeypatch, route)
    qkv, ls, bias, mask, pad, ref = _windowed_case(name)
    row_map, B_ = hip.window_slice_map(B, D_, H_, W_, ws, ss, DEV)
    nW = mask.shape[0] if mask is not None else 1
    assert B_ == B * 6 and (mask is None or B_ % nW == 0) and int((row_map < 0).sum()) > 0
    run = lambda: _run_ann((qkv, ls, bias, mask), NH_, nW, row_map=row_map, pad=pad, B_=B_, N=N, rows=qkv.shape[0])
    _check_ann(run, ref, _expected_kernel(route, N), N, mask is not None, B_, NH_, f"windowed {name} {route}")


def test_wrappers_run_the_same_call(monkeypatch):
    """hip.win_attn_ann / win_attn_sew / win_attn_ann_windowed fill the descriptor as this file does: bit-equal results."""
    _switch(monkeypatch, "default")
    N, (B_, nH, nW) = 114, TILED[114]
    qkv, ls, bias, mask, _ = _ann_case(N, B_, nH, nW, True)
    got, _ = _run_ann((qkv, ls, bias, mask), nH, nW)
    t = _dev(qkv, ls.reshape(-1), bias, mask)
    assert torch.equal(hip.win_attn_ann(*t, nH).cpu().view(B_ * N, -1), got)
    q, k, v, scale, bias, mask, _, _ = _sew_case(2, N // 2, B_, nH, nW, True)
    got, _ = _run_sew((q, k, v, scale, bias, mask), 2, N // 2, B_, nH, nW)
    t = _dev(q, k, v, scale, bias, mask)
    assert torch.equal(hip.win_attn_sew(*t, nH, 2, B_, N // 2).cpu().view(B_ * N, -1), got)
    B, ws, ss, _ = WINDOWED["w9_shift"]
    qkv, ls, bias, mask, pad, _ = _windowed_case("w9_shift")
    row_map, B_ = hip.window_slice_map(B, D_, H_, W_, ws, ss, DEV)
    got, _ = _run_ann((qkv, ls, bias, mask), NH_, mask.shape[0], row_map=row_map, pad=pad, B_=B_, N=162, rows=qkv.shape[0])
    t = _dev(qkv, ls.reshape(-1), bias, mask, pad)
    assert torch.equal(hip.win_attn_ann_windowed(t[0], row_map, B_, 162, t[4], t[1], t[2], t[3], NH_).cpu(), got)
