"""sdf_spike_conv2d_fwd and sdf_spike_conv2d_multi_fwd on every route their dispatcher can take (csrc/spike_gemm.hip,
csrc/spike_conv_wres.hip, csrc/spike_mm_pp.hip), against float64 references (tests/spike_conv_cases.py).

Four kernel families sit behind the entry points: the weight-resident kernel on 16-bit planes spike_conv_wres_kernel<NSPLIT, TT, 6>,
the weight-resident kernel on digit planes spike_conv_wres_i8_kernel<TT, CIN16, RB, NGRP, S2, KH, SPK>, the ping-pong kernel with the
im2col loader spike_mm_pp_kernel<NSPLIT, TT, true> (with splitk_reduce_kernel behind its split-K plan) and spike_mm_pp_multi_kernel<NSPLIT>.
Every GPU case

  * names its route LITERALLY in its table - kernel, template arguments, threads, workgroups, whether a reduce pass follows - and asserts
    through hip.launch_log() that exactly those launches happened, in that order; the comment beside a row derives the workgroups;
  * writes `out` / `out_spike` into slices of larger buffers: 64 guard rows on each side, NaN (fp32) or the byte 7 (spikes) everywhere
    beforehand; afterwards the guards, and the rows a row map does not name or drops, hold the same bits, and no NaN / 7 is left where
    a result belongs; the operand has a guard image of ones on each side (a tap outside an image must read zero);
  * runs the call twice: bit-equal.

References.  EXACT cases: torch.equal with the float64 product (the premise is asserted on the CPU below).  RANDOM fp32 cases: per
element |got - ref64| <= GAMMA[kernel] * mag, mag = |alpha| conv(A, |W|) + |beta| + |resid|, and exactly 0 where mag is 0 (the silent
image, the column with alpha = beta = 0).  FUSED-NEURON cases with a membrane output: the membrane to that bound, the spikes equal to
oracle.neuron_ref of the kernel's OWN membrane bit for bit.  SPIKES-ONLY forms: O.delta_consistent on the float64 pre-activation cast
to fp32, delta = 16 * 2^-23 * max(rms, v_th): 0 unexplained decisions, at most 1e-4 of them ambiguous, rate in (0.03, 0.97); on digit
planes also bit-equal to the spikes of the membrane form of the same case (exact integer sums, the same arithmetic).

Which test covers which instantiation:
  spike_conv_wres_kernel<1|2, 0, 6>                       test_wres16_f32, test_wres16_f32_epilogue, test_default_16bit_*
  spike_conv_wres_kernel<1|2, 10, 6>                      test_wres16_fused
  spike_conv_wres_i8_kernel<0, 6, 1, 2>                   test_wres8_f32, test_wres8_f32_epilogue, test_wres8_default_tile_rule (85 images), test_wres8_grid_rule
  spike_conv_wres_i8_kernel<0, 6, 2, 2>                   test_wres8_f32_16_row_tile, test_wres8_default_tile_rule (86 images)
  spike_conv_wres_i8_kernel<10, 6, 1, 3, false, 1, true>  test_wres8_fused (spikes only), test_wres8_fused_three_group_grid
  spike_conv_wres_i8_kernel<10, 6, 1, 3>                  test_wres8_fused (membrane), test_wres8_fused_switches (SDF_CONV_WRES_NOSPK=1)
  spike_conv_wres_i8_kernel<10, 6, 1, 2>                  test_wres8_fused_switches (SDF_CONV_WRES_GROUPS=2)
  spike_conv_wres_i8_kernel<10, 6, 2, 2>                  test_wres8_fused_16_row_tile
  spike_conv_wres_i8_kernel<0, 3, 1, 2, true>             test_wres8_stride2_f32, test_wres8_stride2_f32_epilogue (48 channels)
  spike_conv_wres_i8_kernel<0, 3, 1, 2, true, 2>          the same two tests (96 channels)
  spike_conv_wres_i8_kernel<10, 3, 1, 3, true>            test_wres8_stride2_fused
  spike_conv_wres_i8_kernel<10, 3, 1, 2, true>            test_wres8_stride2_fused (SDF_CONV_WRES_GROUPS=2)
  spike_mm_pp_kernel<1|2|3, 0, true> + reduce             test_pp_f32_splitk, test_pp_f32_splitk_epilogue, test_pp_parity_classes, test_multi_falls_back, test_default_16bit_*
  spike_mm_pp_kernel<1|2|3, 0, true> without split-K      test_pp_f32_no_splitk, test_multi_one_launch (SDF_CONV_MULTI=0)
  spike_mm_pp_kernel<1|2|3, 10, true>                     test_pp_fused, test_default_16bit_fused_takes_pingpong
  spike_mm_pp_multi_kernel<1|2|3>                         test_multi_one_launch
Left out on purpose: the image-chunk loop of sdf_spike_conv2d_fwd needs operands beyond 2^31 bytes, which no test of a few seconds can
hold.  The small-M and the wide kernel keep their own files (test_smallm_gpu.py, test_wide_conv_gpu.py).

Measured on an MI355X (all random cases of this file, fp32 results and membranes), largest |err| / mag per kernel and weight format
(1 / 2 / 3 planes; digits):
  spike_conv_wres_kernel       6.0e-8 / 1.8e-7 / -          -> GAMMA 2^-20 (9.5e-7): the smallest power of two >= 4 x 1.8e-7
  spike_conv_wres_i8_kernel    digits 8.555e-8              -> GAMMA 2^-21 (4.8e-7): exact integer sums; 2^-24 in the fp32 forms, the
                               largest figure is a stride-2 membrane (the digits' fp32 sum and the BN fma round separately)
  spike_mm_pp_kernel           6.0e-8 / 1.8e-7 / 1.8e-7     -> GAMMA 2^-20
  splitk_reduce_kernel         6.0e-8 / 1.3e-7 / 1.4e-7     -> GAMMA 2^-20
  spike_mm_pp_multi_kernel     7.45e-8 / 2.08e-7 / 2.432e-7 -> GAMMA 2^-19 (1.9e-6): 4 x 2.432e-7 = 9.73e-7 is above 2^-20 = 9.54e-7
                               (the body of spike_mm_pp_kernel; the figures are given unrounded so that the rule can be checked)
(the factor 4 covers other accumulation orders when a tile shape changes; all far below the project's 1e-5 for these products).
Fused neuron, spikes-only forms: 18.2 M decisions in 137 runs (10.6 M on the digit kernel, 2.4 M on the 16-bit weight-resident kernel,
5.2 M on the ping-pong kernel), 42 of them ambiguous (19 / 7 / 16), 0 differ from the reference's, 0 unexplained.
Run time there: the 384 GPU cases in 7.5 s together; the slowest (the default tile rule: two results of 19 MB compared element by
element on the host) 0.51 s, a multi launch of 50 MB 0.34 s, everything else below 0.25 s.
"""
import functools

import pytest
import torch

import spike_conv_cases as C
import spike_gemm_cases as G
from sdformerflow_amd import hip

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD = C.GUARD
WRES, WRES8, PP, REDUCE, MULTI = ("spike_conv_wres_kernel", "spike_conv_wres_i8_kernel", "spike_mm_pp_kernel", "splitk_reduce_kernel",
                                  "spike_mm_pp_multi_kernel")
GAMMA = {WRES: 2.0 ** -20, WRES8: 2.0 ** -21, PP: 2.0 ** -20, REDUCE: 2.0 ** -20, MULTI: 2.0 ** -19}      # from the measured figures above
assert max(GAMMA.values()) <= 1e-5
SWITCHES = {"wres": "SDF_CONV_WRES", "rb": "SDF_CONV_WRES_RB", "groups": "SDF_CONV_WRES_GROUPS", "nospk": "SDF_CONV_WRES_NOSPK",
            "cb_inner": "SDF_CONV_WRES_CB_INNER", "multi": "SDF_CONV_MULTI", "pair": "SDF_PP_PAIR", "ksplit": "SDF_KSPLIT_MULT",
            "smallm": "SDF_SMALLM", "wide": "SDF_WIDE_CONV"}
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()


def w16(ns, tt, wgs):
    return (WRES, (ns, tt, 6), 512, wgs)


def w8(targs, threads, wgs):
    """spike_conv_wres_i8_kernel<TT, CIN16, RB, NGRP, S2 = false, KH = 1, SPK = false>"""
    return (WRES8, tuple(targs) + (False, 1, False)[len(targs) - 4:], threads, wgs)


def pp(ns, tt, wgs):
    return (PP, (ns, tt, True), 768, wgs)


def reduce(wgs):
    return (REDUCE, None, 256, wgs)


def multi(ns, wgs):
    return (MULTI, (ns,), 768, wgs)


def _assert_launches(log, want):
    """Exactly the launches `want`, in order: (kernel, template arguments, threads, workgroups) each; the demangled or the mangled name."""
    assert len(log.rows) == len(want), (log.rows, want)
    for (name, wgs, threads, _, _), (kernel, targs, wthreads, wwgs) in zip(log.rows, want):
        names = (kernel, kernel)
        if targs is not None:
            dem = ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in targs)
            man = "".join(f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in targs)
            names = (f"{kernel}<{dem}>", f"{kernel}I{man}E")
        assert names[0] in name or names[1] in name, (name, names)
        assert (threads, wgs) == (wthreads, wwgs), (name, threads, wgs, wthreads, wwgs)


def _route(monkeypatch, **env):
    for s in SWITCHES.values():
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(SWITCHES[k], str(v))


@functools.lru_cache(maxsize=None)
def _planes(wkey):
    W = C.weights(*wkey).to(DEV)
    return hip.split_weight_i8x3(W) if wkey[2] == "i8" else hip.split_weight(W, wkey[2])


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


# ---------------------------------------------------------------------------------------------------- fp32 epilogue
def _run_f32(c, lay, Wp):
    rows, f = c["rows"], c["flags"]
    buf = lay["init"].to(DEV)
    out = buf[GUARD:GUARD + rows]
    resid = out if "res_in" in f else None
    if "res_sep" in f:
        rbuf = lay["resid"].to(DEV)
        resid = rbuf[GUARD:GUARD + rows]
    x = c["abuf"].to(DEV)[1:c["imgs"] + 1]
    alpha, beta = _dev(c["alpha"]), _dev(c["beta"])
    rowmap = c["dst"].to(torch.int32).to(DEV) if "map" in f else None
    KH, KW, dy, dx = c["taps"]
    with hip.launch_log() as log:
        hip.spike_conv2d(x, Wp, c["imgs"], c["H"], c["W"], c["Cin"], c["OH"], c["OW"], KH, KW, c["stride"], dy, dx, out=out, alpha=alpha,
                         beta=beta, resid=resid, out_rowmap=rowmap)
    torch.cuda.synchronize()
    return buf.cpu(), log


def _compare_f32(got, lay, exact, kernel, what, silent=False):
    w = lay["written"]
    assert torch.equal(got.view(torch.int32)[~w], lay["init"].view(torch.int32)[~w]), "a store outside the rows of the result"
    res, ref = got[w], lay["ref"][w]
    assert not torch.isnan(res).any(), "an element of the result was never written"
    if exact:
        assert torch.equal(res, ref.float()), f"{int((res != ref.float()).sum())} of {res.numel()} elements differ from the exact product"
        return
    mag = lay["mag"][w]
    zero = mag == 0
    assert bool((res[zero] == 0).all()), "an element without any term is not exactly 0"
    if silent:
        assert bool(zero.any())                                             # (the silent image)
    ratio = ((res.double() - ref).abs()[~zero] / mag[~zero]).max().item()
    print(f"\nSCONV f32 {kernel} {what} err/mag {ratio:.3e}")
    assert ratio <= GAMMA[kernel], ratio


def _check_f32(monkeypatch, env, want, imgs, H, W, Cin, N, fmt, stride=1, feat="plain", exact=False):
    _route(monkeypatch, **env)
    c = C.f32_case(imgs, H, W, Cin, N, fmt, stride, feat, exact)
    lay = G.f32_layout(c)
    Wp = _planes(c["wkey"])
    got, log = _run_f32(c, lay, Wp)
    _assert_launches(log, want)
    _compare_f32(got, lay, exact, want[-1][0], f"fmt{fmt} {imgs}x{H}x{W}x{Cin}->{N} s{stride} {feat}", silent=feat == "plain" and imgs > 1)
    again, _ = _run_f32(c, lay, Wp)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"
    return got


EXACT = pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])

# weight-resident kernel, 16-bit planes (SDF_CONV_WRES=2), Cin 96, stride 1, tiles of 8 x 16 pixels x 32 columns: (imgs, H, W, N, workgroups)
W16_F32 = [(1, 1, 1, 32, 1),            # 1 image x 1 tile x 1 column block
           (2, 9, 17, 64, 16),          # ceil(9/8) * ceil(17/16) = 2 * 2 tiles an image, partial in both directions: 2 * 4 tiles x 2 column blocks
           (11, 9, 17, 192, 256)]       # 11 * 4 = 44 tiles x 6 column blocks = 264 items on min(264, 256) workgroups: eight walk two


@gpu
@EXACT
@pytest.mark.parametrize("ns", (1, 2))
@pytest.mark.parametrize("imgs,H,W,N,wgs", W16_F32)
def test_wres16_f32(monkeypatch, imgs, H, W, N, wgs, ns, exact):
    _check_f32(monkeypatch, dict(wres=2), [w16(ns, 0, wgs)], imgs, H, W, 96, N, ns, exact=exact)


@gpu
@pytest.mark.parametrize("feat", ("bn", "res_sep", "res_in"))
@pytest.mark.parametrize("ns", (1, 2))
def test_wres16_f32_epilogue(monkeypatch, ns, feat):
    _check_f32(monkeypatch, dict(wres=2), [w16(ns, 0, 16)], 2, 9, 17, 96, 64, ns, feat=feat)


# weight-resident kernel, digit planes (the default route of these shapes), 8-row tile: (imgs, H, W, N, workgroups)
W8_F32 = [(1, 1, 1, 32, 1),
          (2, 9, 17, 64, 16),           # 8 tiles x 2 column blocks = 16 items < 64: one workgroup each
          # 44 tiles x 6 = 264 items >= 64: two wave groups, rounds = ceil(264 / 512) = 1, per = 2 items a workgroup; tile ranges
          # nr = ceil(44 / 2) = 22 -> 22 * 6 = 132 is no multiple of 8 -> 23 (138) -> 24: 144 workgroups, column blocks side by side
          (11, 9, 17, 192, 144)]


@gpu
@EXACT
@pytest.mark.parametrize("imgs,H,W,N,wgs", W8_F32)
def test_wres8_f32(monkeypatch, imgs, H, W, N, wgs, exact):
    _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, wgs)], imgs, H, W, 96, N, "i8", exact=exact)


@gpu
@pytest.mark.parametrize("feat", ("bn", "res_sep", "res_in"))
def test_wres8_f32_epilogue(monkeypatch, feat):
    _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, 16)], 2, 9, 17, 96, 64, "i8", feat=feat)


@gpu
@pytest.mark.parametrize("imgs,H,W,N,wgs", W8_F32)
def test_wres8_f32_exact_on_all_three_digits(monkeypatch, imgs, H, W, N, wgs):
    """Exact weights on a grid of 2^-26 (C.weights, exact = "fine"): d0, d1 and d2 all carry bits, the result is the float64 product."""
    _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, wgs)], imgs, H, W, 96, N, "i8", exact="fine")


# 16-row tile (SDF_CONV_WRES_RB=2): (imgs, H, W, N, workgroups)
W8_RB2 = [(2, 17, 17, 64, 16),          # ceil(17/16) * ceil(17/16) = 4 tiles an image: 8 tiles x 2 column blocks
          (2, 9, 17, 64, 8)]            # 1 * 2 tiles an image: 4 tiles x 2; the second row block of every tile lies outside the image


@gpu
@pytest.mark.parametrize("feat,exact", [("plain", True), ("plain", False), ("res_in", False)], ids=("exact", "random", "res_in"))
@pytest.mark.parametrize("imgs,H,W,N,wgs", W8_RB2)
def test_wres8_f32_16_row_tile(monkeypatch, imgs, H, W, N, wgs, feat, exact):
    _check_f32(monkeypatch, dict(rb=2), [w8((0, 6, 2, 2), 512, wgs)], imgs, H, W, 96, N, "i8", feat=feat, exact=exact)


@gpu
@pytest.mark.parametrize("imgs,H,W,N,wgs", W8_RB2)
def test_wres8_f32_16_row_tile_exact_on_all_three_digits(monkeypatch, imgs, H, W, N, wgs):
    _check_f32(monkeypatch, dict(rb=2), [w8((0, 6, 2, 2), 512, wgs)], imgs, H, W, 96, N, "i8", exact="fine")


@gpu
def test_wres8_default_tile_rule(monkeypatch):
    """No switch: 16-row tiles from items16 = imgs * ceil(OH/16) * ceil(OW/16) * N/32 >= 2048 on.
    86 images of 17 x 17, N = 192: items16 = 86 * 2 * 2 * 6 = 2064 -> 16-row tiles: 344 tiles x 6 = 2064 items, rounds = ceil(2064 / 512) = 5,
    per = 10; nr = ceil(344 / 10) = 35 -> 35 * 6 = 210 is no multiple of 8 -> 36: 216 workgroups.
    85 images: items16 = 2040 -> 8-row tiles: 85 * 3 * 2 = 510 tiles x 6 = 3060 items, rounds = 6, per = 12: ceil(3060 / 12) = 255 workgroups;
    nr = ceil(510 / 12) = 43 -> 43 * 6 = 258 > 256: the column-block-inner mapping does not fit, 255 stays."""
    _check_f32(monkeypatch, {}, [w8((0, 6, 2, 2), 512, 216)], 86, 17, 17, 96, 192, "i8")
    _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, 255)], 85, 17, 17, 96, 192, "i8")


@gpu
def test_wres8_grid_rule(monkeypatch):
    """23 images of 9 x 17, N = 192: 92 tiles x 6 = 552 items, rounds = ceil(552 / 512) = 2, per = 4.  Column blocks inner (default):
    nr = ceil(92 / 4) = 23 -> 138 is no multiple of 8 -> 24 ranges x 6 = 144 workgroups.  SDF_CONV_WRES_CB_INNER=0: ceil(552 / 4) = 138.
    The integer sums are exact and the epilogue is per element: the two mappings give the same bits."""
    a = _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, 144)], 23, 9, 17, 96, 192, "i8", feat="bn")
    b = _check_f32(monkeypatch, dict(cb_inner=0), [w8((0, 6, 1, 2), 512, 138)], 23, 9, 17, 96, 192, "i8", feat="bn")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# stride 2 on digit planes: inputs 1 x 1 | 16 x 32 (one 8 x 16 output tile) | 17 x 33 (9 x 17 outputs: ragged) | 18 x 34 (9 x 17 outputs,
# the last input row and column a tap of the last outputs).  2 images; workgroups = 2 * tiles an image * N / 32: (H, W, N, workgroups)
S2_SHAPES = [(1, 1, 96, 6), (16, 32, 96, 6), (17, 33, 96, 24), (18, 34, 96, 24),           # 2 * (1 | 1 | 4 | 4) tiles x 3 column blocks
             (1, 1, 64, 4), (16, 32, 64, 4), (17, 33, 64, 16), (18, 34, 64, 16)]           # ... x 2 column blocks


@gpu
@EXACT
@pytest.mark.parametrize("Cin", (48, 96))
@pytest.mark.parametrize("H,W,N,wgs", S2_SHAPES)
def test_wres8_stride2_f32(monkeypatch, H, W, N, wgs, Cin, exact):
    targs = (0, 3, 1, 2, True) if Cin == 48 else (0, 3, 1, 2, True, 2)         # 96 channels: two channel passes of 48
    _check_f32(monkeypatch, {}, [w8(targs, 512, wgs)], 2, H, W, Cin, N, "i8", stride=2, exact=exact)


@gpu
@pytest.mark.parametrize("Cin", (48, 96))
def test_wres8_stride2_f32_exact_on_all_three_digits(monkeypatch, Cin):
    targs = (0, 3, 1, 2, True) if Cin == 48 else (0, 3, 1, 2, True, 2)
    _check_f32(monkeypatch, {}, [w8(targs, 512, 24)], 2, 17, 33, Cin, 96, "i8", stride=2, exact="fine")


@gpu
@pytest.mark.parametrize("Cin", (48, 96))
@pytest.mark.parametrize("feat", ("bn", "res_in"))
def test_wres8_stride2_f32_epilogue(monkeypatch, feat, Cin):
    targs = (0, 3, 1, 2, True) if Cin == 48 else (0, 3, 1, 2, True, 2)
    _check_f32(monkeypatch, {}, [w8(targs, 512, 24)], 2, 17, 33, Cin, 96, "i8", stride=2, feat=feat)


# ping-pong kernel with the im2col loader (SDF_CONV_WRES=0): tiles of 256 rows x 96 columns, K stages of 64.  Split-K (at most 128 tiles,
# S >= 4 stages): the chunk count ks <= min(S / 2, 32) with the least rounds * (ceil(S / ks) + 3), the first of equals.
#   Cin 48:  K = 432, S = 7 (6 stages + 48): ks = 1, 2, 3 cost 10, 7, 6 -> 3 chunks of 3 stages
#   Cin 112: K = 1008, S = 16 (15 stages + 48): ks = 1 .. 8 cost 19, 11, 9, 7, 7, 6, 6, 5 -> 8 chunks of 2 stages
# items = tiles * ks on one workgroup each below 16 items, on ceil(items / 2) from 16 on (a workgroup's two consumer groups alternate);
# the reduce pass has M * N / 4 quads on ceil(. / 256) workgroups.  (imgs, H, W, Cin, N, stride, pp workgroups, reduce workgroups)
PP_SPLITK = [(1, 1, 1, 48, 96, 1, 3, 1),             # M = 1: 1 tile x 3 chunks; 24 quads
             (1, 1, 1, 48, 288, 1, 9, 1),            # 3 tiles x 3; 72 quads
             (1, 1, 257, 48, 96, 1, 6, 25),          # M = 257: 2 tiles x 3; 257 * 24 = 6168 quads
             (1, 1, 257, 48, 288, 1, 9, 73),         # 6 tiles x 3 = 18 items on 9; 257 * 72 = 18504 quads
             (1, 1, 1, 112, 96, 1, 8, 1),            # 1 tile x 8
             (1, 1, 1, 112, 288, 1, 12, 1),          # 3 tiles x 8 = 24 items on 12
             (1, 1, 257, 112, 96, 1, 8, 25),         # 2 tiles x 8 = 16 items on 8
             (1, 1, 257, 112, 288, 1, 24, 73),       # 6 tiles x 8 = 48 items on 24
             (2, 9, 17, 48, 96, 2, 3, 9)]            # stride 2: 2 images of 5 x 9 outputs, M = 90: 1 tile x 3; 90 * 24 = 2160 quads
NS = (1, 2, 3)


@gpu
@EXACT
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("imgs,H,W,Cin,N,stride,wgs,rwgs", PP_SPLITK)
def test_pp_f32_splitk(monkeypatch, imgs, H, W, Cin, N, stride, wgs, rwgs, ns, exact):
    _check_f32(monkeypatch, dict(wres=0), [pp(ns, 0, wgs), reduce(rwgs)], imgs, H, W, Cin, N, ns, stride=stride, exact=exact)


@gpu
@pytest.mark.parametrize("feat", ("bn", "res_sep", "res_in", "map", "all"))
@pytest.mark.parametrize("ns", NS)
def test_pp_f32_splitk_epilogue(monkeypatch, ns, feat):
    """Every epilogue feature in the reduce pass: 2 images of 9 x 17 at stride 1, M = 306: 2 tiles x 3 chunks = 6 items; 306 * 24 = 7344 quads."""
    _check_f32(monkeypatch, dict(wres=0), [pp(ns, 0, 6), reduce(29)], 2, 9, 17, 48, 96, ns, feat=feat)


@gpu
@pytest.mark.parametrize("ns", NS)
def test_pp_f32_no_splitk(monkeypatch, ns):
    """3 images of 60 x 60, N = 288: M = 10 800 -> 43 row tiles x 3 column blocks = 129 tiles > 128: no split-K.  129 items in pairs:
    rounds = ceil(129 / 512) = 1, ceil(129 / 2) = 65 workgroups (one of them with a single item); SDF_PP_PAIR=0: one item each, 129."""
    a = _check_f32(monkeypatch, dict(wres=0), [pp(ns, 0, 65)], 3, 60, 60, 48, 288, ns, feat="all")
    b = _check_f32(monkeypatch, dict(wres=0, pair=0), [pp(ns, 0, 129)], 3, 60, 60, 48, 288, ns, feat="all")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- taps, row maps, the multi launch
def _device_classes(dc, ns):
    """engine.deconv_classes on the case's weight, with the case's row maps (dropped rows included)."""
    from sdformerflow_amd.engine import deconv_classes
    cls = deconv_classes(dc["w"].to(DEV), dc["imgs"], dc["H"], dc["W"], dc["cp"], ns, DEV)
    out = []
    for d, cl in zip(cls, dc["classes"]):
        assert (d["KH"], d["KW"], tuple(d["dy"]), tuple(d["dx"])) == cl["taps"]
        assert torch.equal(d["rowmap"].cpu().long(), cl["full"])
        out.append(dict(d, rowmap=cl["dst"].to(torch.int32).to(DEV)))
    return out


# the four parity classes on 200 channels padded to 208, 2 images of 5 x 5 (M = 50: 1 tile), N = 96; 50 * 24 = 1200 quads on 5 workgroups.
#   K = 208 (1 x 1 tap):  S = 4:  ks <= 2,  cost 7, 5 -> 2 chunks
#   K = 416 (1 x 2, 2 x 1): S = 7: 3 chunks (as above)
#   K = 832 (2 x 2):      S = 13: ks <= 6, cost 16, 10, 8, 7, 6, 6 -> 5 chunks
CLASS_WGS = (2, 3, 3, 5)


@gpu
@pytest.mark.parametrize("feat", ("map", "all"))
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("k", range(4))
def test_pp_parity_classes(monkeypatch, k, ns, feat):
    """Each class of engine.deconv_classes on its own (KH / KW in {1, 2} with their own dy / dx, a row map with dropped rows); the CPU
    test below ties the classes' references to conv_transpose2d in float64."""
    _route(monkeypatch, wres=0)
    dc = C.deconv_case(2, 5, 5, 200, 208, 96, ns)
    c = C.class_case(dc, k, feat)
    lay = G.f32_layout(c)
    Wp = _device_classes(dc, ns)[k]["Wp"]
    got, log = _run_f32(c, lay, Wp)
    _assert_launches(log, [pp(ns, 0, CLASS_WGS[k]), reduce(5)])
    _compare_f32(got, lay, False, REDUCE, f"fmt{ns} class {k} {feat}")
    again, _ = _run_f32(c, lay, Wp)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"


def _run_multi(dc, lay, classes, alpha, beta):
    buf = lay["init"].to(DEV)
    x = dc["abuf"].to(DEV)[1:dc["imgs"] + 1]
    with hip.launch_log() as log:
        hip.spike_conv2d_multi(x, classes, dc["imgs"], dc["H"], dc["W"], dc["cp"], dc["H"], dc["W"], buf[GUARD:GUARD + dc["rows"]], alpha=alpha,
                               beta=beta)
    torch.cuda.synchronize()
    return buf.cpu(), log


def _check_multi(monkeypatch, dc, ns, want_one, want_four, bound):
    alpha, beta = C.bn(dc["N"], 5850)
    lay = C.union_layout(dc, alpha, beta)
    classes = _device_classes(dc, ns)
    al, be = alpha.to(DEV), beta.to(DEV)
    _route(monkeypatch, wres=0)
    got, log = _run_multi(dc, lay, classes, al, be)
    _assert_launches(log, want_one)
    _compare_f32(got, lay, False, bound, f"fmt{ns} multi {dc['imgs']}x{dc['H']}x{dc['W']}")
    again, _ = _run_multi(dc, lay, classes, al, be)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"
    _route(monkeypatch, wres=0, multi=0)
    four, log = _run_multi(dc, lay, classes, al, be)
    _assert_launches(log, want_four)
    assert torch.equal(got.view(torch.int32), four.view(torch.int32)), "one launch and four launches differ"


@gpu
@pytest.mark.parametrize("ns", NS)
def test_multi_one_launch(monkeypatch, ns):
    """4 images of 52 x 52 on 48 channels, N = 288: M = 10 816 -> 43 row tiles x 3 column blocks = 129 tiles a class > 128: no class splits
    K, each plans ceil(129 / 2) = 65 workgroups: ONE launch of 4 * 65 = 260.  SDF_CONV_MULTI=0: four launches of 65, in class order."""
    dc = C.deconv_case(4, 52, 52, 48, 48, 288, ns)
    _check_multi(monkeypatch, dc, ns, [multi(ns, 260)], [pp(ns, 0, 65)] * 4, MULTI)


@gpu
@pytest.mark.parametrize("ns", NS)
def test_multi_falls_back(monkeypatch, ns):
    """10 images of 12 x 16 on 200 (208) channels, N = 96: M = 1920 -> 8 tiles a class <= 128 and S >= 4: every class splits K, which the
    multi kernel does not do - the library launches one by one, in class order: K = 208: 2 chunks, 16 items on 8 workgroups; K = 416:
    3 chunks, 24 on 12; K = 832: 5 chunks, 40 on 20; each followed by its reduce pass of 1920 * 24 = 46 080 quads on 180."""
    dc = C.deconv_case(10, 12, 16, 200, 208, 96, ns)
    want = [pp(ns, 0, 8), reduce(180), pp(ns, 0, 12), reduce(180), pp(ns, 0, 12), reduce(180), pp(ns, 0, 20), reduce(180)]
    _check_multi(monkeypatch, dc, ns, want, want, REDUCE)


# ---------------------------------------------------------------------------------------------------- fused neuron
def _run_sn(c, Wp, memb):
    rows, N = c["imgs"] * c["OH"] * c["OW"], c["N"]
    sbuf = torch.full((GUARD + rows + GUARD, N), 7, dtype=torch.uint8, device=DEV)
    mbuf = torch.full((GUARD + rows + GUARD, N), float("nan"), device=DEV) if memb else None
    p = hip.NeuronParams(c["neuron"], C.TAU, c["v_th"], c["v_reset"], _dev(c["psn_w"]), _dev(c["psn_b"]))
    x = c["abuf"].to(DEV)[1:c["imgs"] + 1]
    alpha, beta, resid = _dev(c["alpha"]), _dev(c["beta"]), _dev(c["resid"])
    KH, KW, dy, dx = c["taps"]
    with hip.launch_log() as log:
        hip.spike_conv2d(x, Wp, c["imgs"], c["H"], c["W"], c["Cin"], c["OH"], c["OW"], KH, KW, c["stride"], dy, dx,
                         out=mbuf[GUARD:GUARD + rows] if memb else None, out_spike=sbuf[GUARD:GUARD + rows], alpha=alpha, beta=beta, resid=resid,
                         sn=p, sn_T=c["T"], pos=c["pos"])
    torch.cuda.synchronize()
    s = sbuf.cpu()
    assert bool((s[:GUARD] == 7).all()) and bool((s[GUARD + rows:] == 7).all()), "a store outside `out_spike`"
    s = s[GUARD:GUARD + rows]
    assert bool((s <= 1).all()), "a spike row was never written"
    m = None
    if memb:
        m = mbuf.cpu()
        bits = m.view(torch.int32)
        assert bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + rows:] == NAN_BITS).all()), "a store outside `out`"
        m = m[GUARD:GUARD + rows]
        assert not torch.isnan(m).any(), "a membrane row was never written"
    return s, m, log


def _check_membrane(c, m, s, kernel, what):
    """The membrane `m` a fused call wrote (rows in image order) against the float64 membrane input of its case, and its spikes `s`
    against the reference neuron run on that membrane."""
    T, B, order = c["T"], c["B"], c["order"]
    mag, ref = c["mag"], c["y64"]
    zero = mag == 0
    assert bool((m[zero] == 0).all()), "a membrane element without any term is not exactly 0"
    ratio = ((m.double() - ref).abs()[~zero] / mag[~zero]).max().item()
    print(f"\nSCONV memb {what} err/mag {ratio:.3e}")
    assert ratio <= GAMMA[kernel], ratio
    own = C.sn_reference(c, C.to_steps(m, T, B, order).contiguous())
    st = C.to_steps(s, T, B, order).float()
    assert torch.equal(st, own), f"{int((st != own).sum())} spikes differ from the reference neuron on the kernel's own membrane"


def _check_sn(monkeypatch, env, want, T, B, H, W, Cin, N, fmt, stride, kind, order, memb, want_memb=None):
    """memb: the form with the fp32 membrane output and a residual.  want_memb (digit planes, spikes only): the launches of the
    membrane form of the SAME case (no residual), whose spikes must be the same bits."""
    _route(monkeypatch, **env)
    c = C.sn_case(T, B, H, W, Cin, N, fmt, stride, kind, order, resid=memb)
    Wp = _planes(c["wkey"])
    s, m, log = _run_sn(c, Wp, memb)
    _assert_launches(log, want)
    st = C.to_steps(s, T, B, order)
    what = f"{want[0][0]} fmt{fmt} T{T} B{B} {H}x{W}x{Cin}->{N} s{stride} {kind} {order}"
    if memb:
        _check_membrane(c, m, s, want[0][0], what)
    else:
        rep = C.sn_report(c, st)
        print(f"\nSCONV sn {what} {rep}")
        assert rep["unexplained"] == 0, rep
        assert rep["ambiguous"] <= 1e-4 * rep["n"], rep
        assert 0.03 < st.float().mean().item() < 0.97
    s2, m2, _ = _run_sn(c, Wp, memb)
    assert torch.equal(s, s2) and (m is None or torch.equal(m.view(torch.int32), m2.view(torch.int32))), "two calls differ"
    if want_memb is not None:
        s3, m3, log = _run_sn(c, Wp, True)
        _assert_launches(log, want_memb)
        _check_membrane(c, m3, s3, want_memb[0][0], what + " (membrane form)")
        assert torch.equal(s, s3), "the spikes-only form and the membrane form differ"


SN_KINDS = ("lif", "lif0", "if")
ORDERS = ("tb", "bt")


@gpu
@pytest.mark.parametrize("memb", (False, True), ids=("spikes", "membrane"))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", SN_KINDS)
@pytest.mark.parametrize("ns", (1, 2))
def test_wres16_fused(monkeypatch, ns, kind, order, memb):
    """T = 10, B = 2, 9 x 17, N = 64 (SDF_CONV_WRES=2): items are (batch element, tile, column block) = 2 * 4 * 2 = 16 workgroups."""
    _check_sn(monkeypatch, dict(wres=2), [w16(ns, 10, 16)], 10, 2, 9, 17, 96, 64, ns, 1, kind, order, memb)


# the digit kernel's fused form at stride 1, B = 2, 9 x 17, N = 64: 2 * 4 tiles x 2 column blocks = 16 items < 64 -> 16 workgroups
SPK3, MEM3, MEM2 = (10, 6, 1, 3, False, 1, True), (10, 6, 1, 3), (10, 6, 1, 2)


@gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", SN_KINDS)
@pytest.mark.parametrize("T", (5, 10, 20))
def test_wres8_fused(monkeypatch, T, kind, order):
    """T = 5, 10 and 20 run the TT = 10 instantiation (the time loop is rolled).  Spikes only: the three-group SPK form, 768 threads -
    and the same bits as the membrane form <10, 6, 1, 3>; with membrane + residual: <10, 6, 1, 3>."""
    args = (T, 2, 9, 17, 96, 64, "i8", 1, kind, order)
    _check_sn(monkeypatch, {}, [w8(SPK3, 768, 16)], *args, False, want_memb=[w8(MEM3, 768, 16)])
    _check_sn(monkeypatch, {}, [w8(MEM3, 768, 16)], *args, True)


@gpu
@pytest.mark.parametrize("T", (5, 10, 20))
def test_wres8_fused_switches(monkeypatch, T):
    """SDF_CONV_WRES_NOSPK=1: spikes only on <10, 6, 1, 3>; SDF_CONV_WRES_GROUPS=2: <10, 6, 1, 2> on 512 threads, both forms."""
    args = (T, 2, 9, 17, 96, 64, "i8", 1, "lif", "bt")
    _check_sn(monkeypatch, dict(nospk=1), [w8(MEM3, 768, 16)], *args, False)
    _check_sn(monkeypatch, dict(groups=2), [w8(MEM2, 512, 16)], *args, False, want_memb=[w8(MEM2, 512, 16)])
    _check_sn(monkeypatch, dict(groups=2), [w8(MEM2, 512, 16)], *args, True)


@gpu
@pytest.mark.parametrize("memb", (False, True), ids=("spikes", "membrane"))
@pytest.mark.parametrize("T", (5, 10))
def test_wres8_fused_16_row_tile(monkeypatch, T, memb):
    """SDF_CONV_WRES_RB=2 at 17 x 17, B = 2, N = 64: 2 * 4 tiles of 16 x 16 x 2 column blocks = 16 workgroups of two wave groups."""
    _check_sn(monkeypatch, dict(rb=2), [w8((10, 6, 2, 2), 512, 16)], T, 2, 17, 17, 96, 64, "i8", 1, "lif", "bt", memb,
              want_memb=None if memb else [w8((10, 6, 2, 2), 512, 16)])


@gpu
def test_wres8_fused_three_group_grid(monkeypatch):
    """T = 5, B = 4, 9 x 17, N = 128: 4 * 4 = 16 tile items x 4 column blocks = 64 items >= 64: three wave groups, rounds =
    ceil(64 / 768) = 1, per = 3 -> ceil(64 / 3) = 22; column blocks inner: nr = ceil(16 / 3) = 6 ranges x 4 = 24, a multiple of 8: 24."""
    _check_sn(monkeypatch, {}, [w8(SPK3, 768, 24)], 5, 4, 9, 17, 96, 128, "i8", 1, "lif", "bt", False, want_memb=[w8(MEM3, 768, 24)])


@gpu
@pytest.mark.parametrize("groups", (3, 2))
@pytest.mark.parametrize("kind", SN_KINDS)
@pytest.mark.parametrize("H,W,N,wgs", S2_SHAPES)
def test_wres8_stride2_fused(monkeypatch, H, W, N, wgs, kind, groups):
    """48 channels at stride 2, T = 5, B = 2 in (b, t) order: B * tiles an image * N / 32 workgroups, as S2_SHAPES has them for 2 images.
    Three wave groups by default, two under SDF_CONV_WRES_GROUPS=2; the stride-2 form has no spikes-only instantiation."""
    want = [w8((10, 3, 1, 3, True), 768, wgs)] if groups == 3 else [w8((10, 3, 1, 2, True), 512, wgs)]
    env = {} if groups == 3 else dict(groups=2)
    _check_sn(monkeypatch, env, want, 5, 2, H, W, 48, N, "i8", 2, kind, "bt", False, want_memb=want)


@gpu
def test_wres8_stride2_fused_with_residual_is_refused(monkeypatch):
    """The stride-2 fused form has no shortcut (spike_conv_wres_plan), and digit planes have no streaming form: SDF_E_SHAPE."""
    _route(monkeypatch)
    c = C.sn_case(5, 2, 17, 33, 48, 96, "i8", 2, "lif", "bt", resid=True)
    with pytest.raises(hip.SdfError) as e:
        _run_sn(c, _planes(c["wkey"]), True)
    assert e.value.rc == hip.E_SHAPE


# ping-pong kernel, fused neuron (SDF_CONV_WRES=0), T = 10 on 48 channels (6 stages + 48): a tile holds 8 * (32 / 10) = 24 positions.
#   B = 1 at 5 x 5, (t, b): 25 positions = a tile plus one -> 2 row tiles;  B = 2 at 5 x 5, (b, t): 50 positions -> 3 row tiles
# (B, order, N, workgroups = row tiles x N / 96)
SN_PP = [(1, "tb", 96, 2), (1, "tb", 288, 6), (2, "bt", 96, 3), (2, "bt", 288, 9)]


@gpu
@pytest.mark.parametrize("memb", (False, True), ids=("spikes", "membrane"))
@pytest.mark.parametrize("kind", ("lif", "lif0", "if", "psn"))
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("B,order,N,wgs", SN_PP)
def test_pp_fused(monkeypatch, B, order, N, wgs, ns, kind, memb):
    _check_sn(monkeypatch, dict(wres=0), [pp(ns, 10, wgs)], 10, B, 5, 5, 48, N, ns, 1, kind, order, memb)


# ---------------------------------------------------------------------------------------------------- what the dispatcher does today
@gpu
@pytest.mark.parametrize("ns", (1, 2))
def test_default_16bit_f32_routes(monkeypatch, ns):
    """No switch, 16-bit planes, 96 channels, stride 1, 9 x 17 images (4 tiles), N = 96 (3 column blocks): 43 images = 172 tiles * 3 = 516
    >= 512: the weight-resident kernel on min(516, 256) workgroups.  42 images = 504 < 512: the ping-pong kernel; M = 6426 -> 26 tiles,
    K = 864: S = 14, ks = 1 .. 7 cost 17, 10, 8, 7, 6, 6, 5 -> 7 chunks: 182 items on 91 workgroups; 6426 * 24 = 154 224 quads on 603."""
    _check_f32(monkeypatch, {}, [w16(ns, 0, 256)], 43, 9, 17, 96, 96, ns)
    _check_f32(monkeypatch, {}, [pp(ns, 0, 91), reduce(603)], 42, 9, 17, 96, 96, ns)


@gpu
@pytest.mark.parametrize("ns", (1, 2))
def test_default_16bit_fused_takes_pingpong(monkeypatch, ns):
    """A fused call on 16-bit planes never takes the weight-resident kernel by default: T = 10, B = 6, 9 x 17, N = 96: 918 positions ->
    39 row tiles of 24 x 1 column block = 39 items in pairs on 20 workgroups."""
    _check_sn(monkeypatch, {}, [pp(ns, 10, 20)], 10, 6, 9, 17, 96, 96, ns, 1, "lif", "bt", False)


@gpu
def test_digit_planes_on_96_channels_never_reach_the_small_m_kernel(monkeypatch):
    """10 images (a multiple of the small-M kernel's T) of few rows: its 64-channel K blocks do not divide 96 - the weight-resident
    kernel runs: 10 * 1 tile x 3 column blocks = 30 workgroups."""
    _check_f32(monkeypatch, {}, [w8((0, 6, 1, 2), 512, 30)], 10, 4, 4, 96, 96, "i8")


@gpu
@pytest.mark.parametrize("fmt", C.FORMATS)
def test_held_weights_are_the_device_planes(fmt):
    """The references multiply by the weights rebuilt on the CPU from the format: they are the planes the library makes, bit for bit."""
    for exact in (False, True):
        W = C.weights(64, 9 * 96, fmt, exact)
        dev = _planes((64, 9 * 96, fmt, exact))
        if fmt == "i8":
            d, sc = C.digit_planes(W)
            assert torch.equal(dev.cpu(), d) and torch.equal(dev.sdf_col_scale.cpu(), sc)
        else:
            assert torch.equal(dev.cpu(), C.plane_bits(W, fmt))
            if fmt == 2:
                assert dev.sdf_acc_scale == 1.0 / C.f16_scale(W)


# ---------------------------------------------------------------------------------------------------- the premises, on the CPU
def _exact_cases():
    out = [(i, H, W, 96, N, ns, 1) for i, H, W, N, _ in W16_F32 for ns in (1, 2)]
    out += [(i, H, W, 96, N, "i8", 1) for i, H, W, N, _ in W8_F32 + W8_RB2]
    out += [(2, H, W, Cin, N, "i8", 2) for H, W, N, _ in S2_SHAPES for Cin in (48, 96)]
    out += [(i, H, W, Cin, N, ns, s) for i, H, W, Cin, N, s, _, _ in PP_SPLITK for ns in NS]
    return out


def _fine_cases():
    return [(i, H, W, 96, N, 1) for i, H, W, N, _ in W8_F32 + W8_RB2] + [(2, 17, 33, Cin, 96, 2) for Cin in (48, 96)]


def test_exact_products_are_representable():
    """The premise of the exact cases: the weights are exact in their format, at most one spike a pixel, and the float64 product and the
    sum of the absolute terms - hence every partial sum in any order - are fp32 numbers on the operands' grid."""
    for imgs, H, W, Cin, N, fmt, stride in _exact_cases():
        c = C.f32_case(imgs, H, W, Cin, N, fmt, stride, "plain", True)
        Wm = C.weights(*c["wkey"])
        assert torch.equal(C.held(*c["wkey"]), Wm.double()), (fmt, "the format does not hold the exact weights")
        assert int(c["abuf"][1:imgs + 1].sum(3).max()) <= 1
        grid, top = (2.0 ** 10, 9 / 8) if fmt == "i8" else (2.0 ** 19, 32.0)
        for v in (c["y"], c["mag"]):
            assert torch.equal(v.float().double(), v)
            assert torch.equal(v * grid, (v * grid).round()) and v.abs().max().item() < top
    W = C.weights(64, 864, "i8", True)
    assert float(W.abs().max()) < 1 / 8 and torch.equal(W * 1024, (W * 1024).round())
    # k / 1024 against the row scale 2^-26 is q = k * 2^16: only the top digit holds bits; the finer set uses all three
    assert [int(p.abs().max()) > 0 for p in C.digit_planes(W)[0]] == [False, False, True]
    for imgs, H, W_, Cin, N, stride in _fine_cases():
        c = C.f32_case(imgs, H, W_, Cin, N, "i8", stride, "plain", "fine")
        Wm = C.weights(*c["wkey"])
        assert torch.equal(C.held(*c["wkey"]), Wm.double())
        assert all(int(p.abs().max()) > 64 for p in C.digit_planes(Wm)[0]) and bool((C.digit_planes(Wm)[1] == 2.0 ** -26).all())
        assert int(c["abuf"][1:imgs + 1].sum(3).max()) <= 1
        for v in (c["y"], c["mag"]):
            assert torch.equal(v.float().double(), v)
            assert torch.equal(v * 2.0 ** 26, (v * 2.0 ** 26).round()) and v.abs().max().item() < 0.25


def test_parity_classes_make_the_transposed_convolution():
    """The four classes' references, scattered by their row maps, are ConvTranspose2d(3, 2, 1, 1) of the same spikes in float64."""
    for imgs, H, W, Cin, cp, N in [(2, 5, 5, 200, 208, 96), (4, 52, 52, 48, 48, 288)]:
        dc = C.deconv_case(imgs, H, W, Cin, cp, N, 3, drop=False)
        A = dc["abuf"][1:imgs + 1]
        assert not A[..., Cin:].any()
        w = torch.stack([C.held_weights(dc["w"][:, :, ky, kx].t().contiguous(), 3).t() for ky in range(3) for kx in range(3)], -1)
        ref = torch.nn.functional.conv_transpose2d(A[..., :Cin].permute(0, 3, 1, 2).double(), w.view(Cin, N, 3, 3), None, 2, 1, 1)
        ref = ref.permute(0, 2, 3, 1).reshape(-1, N)
        got = torch.full_like(ref, float("nan"))
        for cl in dc["classes"]:
            got[cl["dst"]] = cl["y"]
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
        assert any((cl["dst"] < 0).any() for cl in C.deconv_case(imgs, H, W, Cin, cp, N, 3)["classes"])


def _fused_cases():
    out = [(10, 2, 9, 17, 96, 64, ns, 1, k, o, m) for ns in (1, 2) for k in SN_KINDS for o in ORDERS for m in (False, True)]
    out += [(T, 2, 9, 17, 96, 64, "i8", 1, k, o, m) for T in (5, 10, 20) for k in SN_KINDS for o in ORDERS for m in (False, True)]
    out += [(T, 2, 17, 17, 96, 64, "i8", 1, "lif", "bt", m) for T in (5, 10) for m in (False, True)]
    out += [(5, 4, 9, 17, 96, 128, "i8", 1, "lif", "bt", False)]
    out += [(5, 2, H, W, 48, N, "i8", 2, k, "bt", False) for H, W, N, _ in S2_SHAPES for k in SN_KINDS]
    out += [(10, B, 5, 5, 48, N, ns, 1, k, o, m) for B, o, N, _ in SN_PP for ns in NS for k in ("lif", "lif0", "if", "psn") for m in (False, True)]
    out += [(10, 6, 9, 17, 96, 96, ns, 1, "lif", "bt", False) for ns in (1, 2)]
    return out


def test_random_fused_cases_are_not_on_the_threshold():
    """The reference's own spikes: at most 1e-4 of a case's decisions are within delta of the threshold, the rate is inside (0.03, 0.97)."""
    for key in sorted(set(_fused_cases()), key=str):
        c = C.sn_case(*key)
        ref = C.sn_reference(c)
        rep = C.sn_report(c, ref)
        assert rep["unexplained"] == 0 and rep["flips"] == 0, (key, rep)
        assert rep["ambiguous"] <= 1e-4 * rep["n"], (key, rep)
        assert 0.03 < ref.mean().item() < 0.97, key
