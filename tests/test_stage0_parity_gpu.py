"""What the stage-0, head and tail kernels COMPUTE, on every instantiation their launch functions can emit: hip.head_conv_sn
(csrc/head_tail.hip launch_head), hip.pred_head (csrc/pred_head.hip sdf_pred_head_fwd), the one-launch first half of hip.qk_attn
(csrc/qk_front.hip launch_qk_front), the one-launch hip.ms_mlp (csrc/ms_mlp_fused.hip launch_t) and hip.qk_gate (csrc/qk_gate.hip),
against CPU references in tests/stage0_cases.py.  tests/test_stage0_routes_gpu.py pins WHICH launches the same entry points make and
compares nothing; this file compares.  Every GPU case

  * asserts the launch it meant to reach - workgroups, threads, kernel, template arguments - through hip.launch_log().  The expected
    line is derived in stage0_cases.py from the dispatch code (launch_head's grid rule, sdf_pred_head_fwd's lanes per position, MlpGeo's
    positions per work item ...) in the notation of tests/golden/stage0_routes.json, not recorded from a run;
  * runs twice into fresh buffers: the same launches, bit-equal results;
  * prefills what the caller allocates with the byte 7 - the next level's spike image of the prediction head, the MLP's workspace with
    its tape, the gate's output between 64 guard rows a side - and requires 7 wherever the call owns nothing.  Outputs the wrappers
    allocate themselves (the head's spikes) are poisoned through the caching allocator (`_poison`);
  * uses neurons of DIFFERENT settings of one class wherever a kernel takes several (stage0_cases.py, "Neurons").

References and bounds (none of them new: exact equality, the 16-ulp delta rule of tests/replay.py with at most 1e-4 of the decisions
ambiguous / 2e-4 flipped, and 1e-5 of the range for fp32 results):
  head convolution   EXACT operands (integers / eighths: every pre-activation exact in fp32 in any order): spikes torch.equal to neuron_ref
                     of the float64 convolution.  RANDOM operands: O.delta_consistent on the float64 pre-activation cast to fp32: 0
                     unexplained decisions, at most 1e-4 ambiguous.  The voxel read in place: bit-equal to the packed call.
  prediction head    spikes and the next level's slices bit-equal to neuron_ref; pred and flow to 1e-5 of their range against float64 on
                     the kernel's own spikes; padding zero, skip slice untouched.
  QK front           (a) q | k, E and the block's output bit-equal to the four-launch form of the entry point; (b) q | k delta-consistent
                     (0 unexplained, at most 2e-4 flipped) with BN(SN_proj(x) W^T) + pe in float64 from neuron_ref's slice spikes and the
                     value the weight planes hold; E bit-equal to k AND SN2_q(head sums of the kernel's own q).  The stacked projection
                     is one product with one neuron by the entry point's contract (include/sdformerflow_hip.h), so sn_k is sn_q there;
                     the separate form has four different neurons.
  MLP                SN1 bit-equal, SN2 delta-consistent on the kernel's own SN1 spikes, the output to 1e-5 of its range on its own SN2
                     spikes (the three steps of test_ms_mlp_fused_gpu.py); tape and no tape give the same x; without the tape the
                     workspace is untouched.
  token gate         e bit-equal to k AND neuron_ref(head sums of q).
The premises - exactness of the EXACT recipe, firing rates inside (0.03, 0.97) (gates: (0.1, 0.9)) and distinct between the settings,
the delta check passed by an fp32 evaluation in the kernel's documented (ky, kx, cin) order, the reference's own spikes passing every
step check, the shapes sitting where the comments say - are the unmarked CPU tests of this file.

Which test covers which instantiation:
  head_conv_mfma_kernel<5|10|20, 2, 48|32|64, true>, <.., 4, 48, true>    test_head_mfma_exact[lif, plif] (all 12), test_head_geometry_exact[mfma_fast],
                                                                          test_head_tile_loop_exact[lif], test_head_voxel_in_place_exact, test_head_random[mfma-lif|plif]
  head_conv_mfma_kernel<.., false> (the same 12)                          test_head_mfma_exact[lif_hard, lif_vr, lif_tau3, if] (all 12 x 4), test_head_geometry_exact[mfma_generic],
                                                                          test_head_tile_loop_exact[lif_vr], test_head_voxel_in_place_exact, test_head_random[mfma-lif_hard ... if]
  head_conv_mfma_psn_kernel<5|10, 2, 48|32>                               test_head_mfma_psn_exact (all 4), test_head_geometry_exact[mfma_psn], test_head_tile_loop_exact[psn],
                                                                          test_head_voxel_in_place_exact[2-mfma_psn], test_head_random[mfma-psn]
  head_conv_sn_kernel<5|10|20, 3|2|4, 2>, <.., 3, 4>                      test_head_16_pixel_exact (all 12 x the seven settings, by W = 48 and by SDF_HEAD_MFMA=0),
                                                                          test_head_geometry_exact[px16, px16_psn], test_head_voxel_in_place_exact, test_head_random[px16-*]
  pred_head_kernel<5|10|20, 8|16|32, 0|1|2> (no <20, .., 1>)              test_pred_head_every_instantiation (all 24), test_pred_head_options (same_next per class, no bias, no pred)
  qk_front_kernel<0|1|2, true|false>                                      test_qk_front (all 6: every case runs with and without the tape)
  ms_mlp_fused_kernel<2, 5|10|20, 6|12, .., 0|1|2, true|false>            test_ms_mlp_one_launch (all 32; PSN has none at T = 20), every case with and without the tape
  ms_mlp_fused_kernel<1|3, 10, 6|12, .., 0|1|2, true|false>               test_ms_mlp_one_launch (all 24)
  qk_gate_kernel (no template; Tq 1 ... 4 and the neuron are run-time)    test_qk_gate
Out of reach of a test this small: nothing of the five launch functions.  Not here on purpose: sizes whose index arithmetic passes
2^31 (the head's host code sends them to the 16-pixel kernel; operands of that size do not fit a test of a second), and the wide-stage
and digit-plane forms of the attention and the MLP (test_ms_wide_gpu.py, test_smallm_gpu.py).

Measured on an MI355X, random cases (decisions / ambiguous under the 16-ulp delta / flips against the reference's own spikes / largest
`needed`, the margin of a decision that followed the kernel against the reference):
  head_conv_mfma_kernel       3 276 800 in 6 cases    / 11 / 0 / 0
  head_conv_mfma_psn_kernel     409 600 in 2 cases    /  0 / 0 / 0
  head_conv_sn_kernel         3 072 000 in 7 cases    / 14 / 0 / 0
  qk_front_kernel (q and k)   4 245 120 in 30 cases   / 17 / 0 / 0
  ms_mlp_fused_kernel (SN2)   4 790 400 in 33 cases   / 14 / 0 / 0
0 unexplained everywhere; the ambiguous counts of the head are those of the CPU premise case by case (they are a property of the
reference and delta).  No kernel took a single decision apart from the reference: nothing here rests on the delta, it is the bound the
issue of this file names.  The exact cases, the prediction head, the token gate, SN1 and E are bit-equal as asserted.
Run time there: the 748 tests of this file (567 on the GPU) in 5.4 s together; the slowest are the three tile-loop cases (23.6 MB
compared on the host, 0.2 - 0.35 s) and the first call of the file (0.36 s), everything else below 0.1 s.
"""
import functools

import pytest
import torch

import stage0_cases as S
from routes_common import logged
from sdformerflow_amd import hip

gpu = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("SDF_HEAD_MFMA", "SDF_QK_FRONT", "SDF_QK_FRONT_ANY", "SDF_MLP_FUSED", "SDF_MLP_FUSED_ANY", "SDF_WIDE", "SDF_RES", "SDF_GEMM_CFG",
            "SDF_GEMM_WS", "SDF_GEMM_WGS")
SIX = tuple(n for n in S.NAMES if n != "psn")


def _route(monkeypatch, **env):
    """the shipped dispatch, but for the switches a case names"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _np(n):
    """a case's neuron for the library (one object per setting: the PSN tables keep their addresses)"""
    if n.psn_w is None:
        return hip.NeuronParams(n.kind, n.tau, n.v_th, n.v_reset)
    return hip.NeuronParams(n.kind, n.tau, n.v_th, n.v_reset, n.psn_w.to(DEV), n.psn_b.to(DEV))


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _poison(shape, dtype, value):
    """Outputs the wrappers allocate themselves come from the caching allocator: a block of the same size, filled with `value` and freed
    right before the call, is normally the one it hands out next - an element the kernel leaves unwritten then shows as `value` (no spike byte is
    7, no result NaN) instead of as an earlier call's correct result."""
    torch.cuda.synchronize()
    t = torch.full(shape, value, dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del t


def _twice(call, want, shape=None, dtype=torch.uint8, value=7):
    """the call run twice into fresh buffers: the launches `want` both times, bit-equal outputs -> the first run's outputs"""
    outs = []
    for _ in range(2):
        if shape is not None:
            _poison(shape, dtype, value)
        got, out = logged(call)
        assert got == want, (got, want)
        outs.append(out)
    for a, b in zip(*outs):
        if a is not None:
            assert a.data_ptr() != b.data_ptr() and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two calls differ"
    return outs[0]


# ==================================================================================================== 1. head convolution
GEO = (2, 3, 64)                                            # (B, H, W) of the coverage cases: 12 tiles of 32 pixels, 3 workgroups


def _head_call(c, n, voxel=None):
    x, bins = (c["x"], None) if voxel is None else voxel
    x, w, al, be = _dev(x), _dev(c["w"]), _dev(c["alpha"]), _dev(c["beta"])
    return lambda: (hip.head_conv_sn(x, w, c["B"], c["T"], c["H"], c["W"], _np(n), al, be, voxel_bins=bins),)


def _head_exact(monkeypatch, T, pair, geo, name, mfma=True, bn=True, env=None):
    _route(monkeypatch, **(env or {}))
    key = (T, pair[0], pair[1]) + tuple(geo) + (True, bn)
    c = S.head_inputs(*key)
    ref, n = S.head_spikes(*key, name)
    want = S.head_route(c, name, mfma and not env)
    (out,) = _twice(_head_call(c, n), want, ref.shape)
    got = out.cpu()
    assert int(got.max()) <= 1, "a spike byte was never written"
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {ref.numel()} spikes differ from the exact reference ({want[0]})"
    return c, n, out


@gpu
@pytest.mark.parametrize("name", SIX)
@pytest.mark.parametrize("pair", S.HEAD_PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("T", S.HEAD_T)
def test_head_mfma_exact(monkeypatch, T, pair, name):
    """head_conv_mfma_kernel<T, Cin, Cout, FAST>: FAST for lif / plif, the written-out generic step for the four class-2 settings"""
    c, _, _ = _head_exact(monkeypatch, T, pair, GEO, name)
    assert ("true>" if name in ("lif", "plif") else "false>") in S.head_route(c, name)[0]


@gpu
@pytest.mark.parametrize("T,pair", sorted(S.HEAD_PSN_MFMA), ids=lambda v: str(v).replace(" ", ""))
def test_head_mfma_psn_exact(monkeypatch, T, pair):
    c, _, _ = _head_exact(monkeypatch, T, pair, GEO, "psn")
    assert "head_conv_mfma_psn_kernel" in S.head_route(c, "psn")[0]


@gpu
@pytest.mark.parametrize("how", ("w48", "switch"))
@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("pair", S.HEAD_PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("T", S.HEAD_T)
def test_head_16_pixel_exact(monkeypatch, T, pair, name, how):
    """head_conv_sn_kernel<T, Cout / 16, Cin>, reached by a width that is no multiple of 32 and by SDF_HEAD_MFMA=0 (PSN at T = 20 and
    on 2 -> 64 / 4 -> 48 has no other kernel)"""
    c, _, _ = _head_exact(monkeypatch, T, pair, (2, 3, 48) if how == "w48" else GEO, name, env={"SDF_HEAD_MFMA": "0"} if how == "switch" else None)
    assert "head_conv_sn_kernel" in S.head_route(c, name, how != "switch")[0]


def test_head_psn_without_a_matrix_pipe_kernel_takes_the_16_pixel_kernel():
    for T in S.HEAD_T:
        for pair in S.HEAD_PAIRS:
            c = {"T": T, "Cin": pair[0], "Cout": pair[1], "B": 2, "H": 3, "W": 64}
            assert ("head_conv_sn_kernel" in S.head_route(c, "psn")[0]) == ((T, pair) not in S.HEAD_PSN_MFMA)


# (B, H, W, BatchNorm): H = 1; both image edges in one tile; three tiles a row; 3 and 7 tiles (idle waves in the last workgroup); no
# BatchNorm; B = 3
HEAD_GEOMETRY = {"h1": (2, 1, 64, True), "w32": (2, 2, 32, True), "w96": (1, 2, 96, True), "tiles3": (1, 3, 32, True), "tiles7": (1, 7, 32, True),
                 "no_bn": (2, 3, 64, False), "b3": (3, 2, 64, True)}
# kernel family -> (T, (Cin, Cout), setting, switches)
HEAD_FAMILY = {"mfma_fast": (10, (2, 48), "plif", None), "mfma_generic": (5, (4, 48), "lif_vr", None), "mfma_psn": (10, (2, 32), "psn", None),
               "px16": (5, (2, 64), "lif_tau3", {"SDF_HEAD_MFMA": "0"}), "px16_psn": (10, (4, 48), "psn", {"SDF_HEAD_MFMA": "0"})}


@gpu
@pytest.mark.parametrize("geo", list(HEAD_GEOMETRY))
@pytest.mark.parametrize("family", list(HEAD_FAMILY))
def test_head_geometry_exact(monkeypatch, family, geo):
    T, pair, name, env = HEAD_FAMILY[family]
    B, H, W, bn = HEAD_GEOMETRY[geo]
    _head_exact(monkeypatch, T, pair, (B, H, W), name, bn=bn, env=env)


# 3 x 205 x 5 = 3075 tiles: above the 768 x 4 a launch holds at once, and no multiple of 4 - three waves take a second tile (the membrane
# starts again), the last workgroup of the first round has one idle wave... the whole 23.6 MB output is compared
LOOP_GEO = (3, 205, 160)


@gpu
@pytest.mark.parametrize("name", ("lif", "lif_vr", "psn"))
def test_head_tile_loop_exact(monkeypatch, name):
    c, _, _ = _head_exact(monkeypatch, 5, (2, 48), LOOP_GEO, name)
    assert S.head_route(c, name)[0].startswith("768 256 0 head_conv_mfma_")


def test_head_tile_loop_case_loops():
    B, H, W = LOOP_GEO
    tiles = B * H * (W // 32)
    assert tiles > 3072 and tiles % 4 and (tiles + 3) // 4 > 768


@gpu
@pytest.mark.parametrize("family", list(HEAD_FAMILY))
@pytest.mark.parametrize("Cin", (2, 4))
def test_head_voxel_in_place_exact(monkeypatch, family, Cin):
    """Cin = 2 from (B, T + 2, 2, H, W), Cin = 4 from (B, 2 T + 1, 2, H, W), the spare bins NaN: bit-equal to the packed NHWC call (and to
    the reference)"""
    T, pair, name, env = HEAD_FAMILY[family]
    pair = {2: pair if pair[0] == 2 else (2, 48), 4: (4, 48)}[Cin]
    c, n, packed = _head_exact(monkeypatch, T, pair, GEO, name, env=env)
    vox = S.head_voxel(c, 2 if Cin == 2 else 1)
    assert vox[1] == (T + 2 if Cin == 2 else 2 * T + 1) and bool(torch.isnan(vox[0]).any())
    (out,) = _twice(_head_call(c, n, vox), S.head_route(c, name, not env), packed.shape)
    assert torch.equal(out, packed)


# RANDOM cases: kernel family x setting, the shapes (T, Cin, Cout) dealt round
HEAD_RSHAPES = ((20, 2, 64), (20, 4, 48), (10, 2, 48), (5, 2, 32))
HEAD_RGEO = (2, 5, 64)
HEAD_RANDOM = [("mfma", n, HEAD_RSHAPES[i % 4]) for i, n in enumerate(SIX)] + [("mfma", "psn", (10, 2, 48)), ("mfma", "psn", (5, 2, 32))] + \
              [("px16", n, HEAD_RSHAPES[(i + 2) % 4]) for i, n in enumerate(S.NAMES)]
_rid = lambda v: f"{v[0]}-{v[1]}-T{v[2][0]}c{v[2][1]}x{v[2][2]}"


@gpu
@pytest.mark.parametrize("case", HEAD_RANDOM, ids=_rid)
def test_head_random(monkeypatch, case):
    family, name, (T, Cin, Cout) = case
    _route(monkeypatch, **({"SDF_HEAD_MFMA": "0"} if family == "px16" else {}))
    key = (T, Cin, Cout) + HEAD_RGEO + (False, True)
    c, n = S.head_inputs(*key), S.head_neuron(name, T, False)
    want = S.head_route(c, name, family == "mfma")
    assert ("mfma" in want[0]) == (family == "mfma")
    shape = (c["B"], T, c["H"], c["W"], Cout)
    (out,) = _twice(_head_call(c, n), want, shape)
    got = out.cpu()
    assert int(got.max()) <= 1
    rep = S.check_report(n.report(c["pre"], got.permute(1, 0, 2, 3, 4)))
    print(f"\nS0PAR head {want[0].split(' ', 3)[3]} {name} n {rep['n']} ambiguous {rep['ambiguous']} flips {rep['flips']} needed {rep['needed']:.3e} delta {rep['delta']:.3e}")


# ---- premises (CPU)
@pytest.mark.parametrize("T", S.HEAD_T)
@pytest.mark.parametrize("pair", S.HEAD_PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_head_exact_premise(T, pair):
    """fp32 conv2d == float64 conv2d, BatchNorm exact, every partial sum on the grid; the seven settings fire at rates inside (0.03, 0.97)
    that differ from one another (two settings that behave alike could not tell a kernel that confuses them)"""
    c = S.head_inputs(T, pair[0], pair[1], *GEO, True, True)
    x, w = c["x"], c["w"]
    assert float(x.abs().max()) == 3 and bool((x == x.round()).all()) and 0.55 < float((x == 0).float().mean()) < 0.7
    assert bool((w * 8 == (w * 8).round()).all()) and float(w.abs().max()) <= 0.5
    assert set(c["alpha"].tolist()) <= {0.5, 1.0, 2.0} and bool((c["beta"] * 16 == (c["beta"] * 16).round()).all())
    y32 = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1)
    y64 = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, 1).permute(0, 2, 3, 1)
    assert torch.equal(y32.double(), y64) and bool((y64 * 8 == (y64 * 8).round()).all()) and float(y64.abs().max()) < 64
    assert torch.equal(c["pre"].double(), c["pre64"]), "BatchNorm is not exact in fp32"
    assert torch.equal(S.head_emulated(c).double(), c["pre64"]), "the fmaf chain in (ky, kx, cin) order is not exact"
    psn = S.head_neuron("psn", T, True)
    assert bool((psn.psn_w * 8 == (psn.psn_w * 8).round()).all()) and float(psn.psn_w.abs().sum(1).max()) * float(c["pre64"].abs().max()) < 2 ** 12
    rates = {name: S.check_rate(S.head_spikes(T, pair[0], pair[1], *GEO, True, True, name)[0]) for name in S.NAMES}
    print("\nS0PAR exact rates", T, pair, {k: round(v, 4) for k, v in rates.items()})
    assert len(set(rates.values())) == len(rates), rates


def test_head_exact_premise_other_geometries():
    for T, pair, name, _ in HEAD_FAMILY.values():
        for B, H, W, bn in list(HEAD_GEOMETRY.values()) + [(2, 3, 48, True)]:
            c = S.head_inputs(T, pair[0], pair[1], B, H, W, True, bn)
            assert torch.equal(c["pre"].double(), c["pre64"]) and (c["alpha"] is None) == (not bn)
            S.check_rate(S.head_spikes(T, pair[0], pair[1], B, H, W, True, bn, name)[0])
    c = S.head_inputs(5, 2, 48, *LOOP_GEO, True, True)
    assert torch.equal(c["pre"].double(), c["pre64"])
    for name in ("lif", "lif_vr", "psn"):
        S.check_rate(S.head_spikes(5, 2, 48, *LOOP_GEO, True, True, name)[0])


@pytest.mark.parametrize("case", HEAD_RANDOM, ids=_rid)
def test_head_random_premise(case):
    """neuron_ref of an fp32 evaluation in the kernel's documented order passes the check the GPU test makes"""
    _, name, (T, Cin, Cout) = case
    c, n = S.head_inputs(T, Cin, Cout, *HEAD_RGEO, False, True), S.head_neuron(name, T, False)
    got = n.ref(S.head_emulated(c))
    rep = S.check_report(n.report(c["pre"], got))
    S.check_rate(got)
    print(f"\nS0PAR premise head {name} T{T} {Cin}x{Cout} n {rep['n']} ambiguous {rep['ambiguous']} flips {rep['flips']} rate {float(got.mean()):.3f}")


def test_head_voxel_layout():
    c = S.head_inputs(5, 4, 48, *GEO, True, True)
    vox, bins = S.head_voxel(c, 1)
    assert bins == 11 and bool(torch.isnan(vox[:, 10]).all()) and not bool(torch.isnan(vox[:, :10]).any())
    # reference patch embedding: channel ci of step t = polarity ci % 2 of bin (ci // 2) T + t
    assert torch.equal(vox[1, 5 + 3, 1], c["x"].view(2, 5, 3, 64, 4)[1, 3, :, :, 3])


# ==================================================================================================== 2. prediction head
def _pred_run(c, want_pred=True):
    B, D, h, w, Cin = c["B"], c["D"], c["h"], c["w"], c["Cin"]
    C2, ld = 32, Cin + 32 + 4 + 12
    z, wgt, bias = _dev(c["z"]), _dev(c["wgt"]), _dev(c["bias"])
    imgs = []

    def call():
        img = torch.full((B, D, h, w, ld), 7, dtype=torch.uint8, device=DEV)
        imgs.append(img)
        pred, flow, sp = hip.pred_head(z, wgt, bias, _np(c["sn"]), c["H"], c["W"], want_pred=want_pred,
                                       nxt=(img, _np(c["sn_next"]), 0, Cin + C2, (Cin + C2 + 4, 12)), keep=True)
        return pred, flow, sp, img
    pred, flow, sp, img = _twice(call, c["route"])
    return (None if pred is None else pred.cpu()), flow.cpu(), sp.cpu(), img.cpu()


def _pred_check(c, pred, flow, sp, img):
    Cin, C2 = c["Cin"], 32
    assert torch.equal(sp.float(), c["sp"]), "SN_pred(z) differs from the oracle"
    S.check_rate(c["sp"])
    p64, f64 = S.pred_reference(c, sp)
    assert flow.shape == f64.shape and (flow.double() - f64).abs().max() <= S.RANGE_TOL * f64.abs().max()
    assert torch.equal(img[..., :Cin].float(), c["next_z"]), "SN_next(z) differs from the oracle"
    S.check_rate(c["next_z"])
    assert int(img[..., Cin + C2 + 2:].sum()) == 0 and bool((img[..., Cin:Cin + C2] == 7).all()), "padding not zero / skip slice touched"
    if pred is not None:
        assert not bool(torch.isnan(pred).any())
        assert torch.equal(pred[..., 2:], torch.zeros_like(pred[..., 2:]))
        assert (pred[..., :2].double() - p64).abs().max() <= S.RANGE_TOL * p64.abs().max()
        assert torch.equal(img[..., Cin + C2:Cin + C2 + 2].float(), S.pred_next_of_pred(c, pred[..., :2])), "SN_next(pred) differs from the oracle"


PRED_ALL = [(D, Cin, cls) for D in S.PRED_D for Cin in S.PRED_CIN for cls in (0, 1, 2) if not (cls == 1 and D == 20)]


def _pred_shape(D, Cin, cls):
    return (S.PRED_D.index(D) * 3 + S.PRED_CIN.index(Cin) + cls) % 4


@gpu
@pytest.mark.parametrize("D,Cin,cls", PRED_ALL)
def test_pred_head_every_instantiation(monkeypatch, D, Cin, cls):
    """pred_head_kernel<D, Cin / 12, class>, sn_next another setting of the class"""
    _route(monkeypatch)
    c = S.pred_case(D, Cin, cls, _pred_shape(D, Cin, cls))
    assert not c["sn"].same_settings(c["sn_next"]) and c["sn"].cls == c["sn_next"].cls == cls
    _pred_check(c, *_pred_run(c))


@gpu
@pytest.mark.parametrize("what", ("same_next0", "same_next1", "same_next2", "no_bias", "no_pred"))
def test_pred_head_options(monkeypatch, what):
    """sn_next identical to sn_pred (z's spikes are computed once), bias = NULL, no prediction output"""
    _route(monkeypatch)
    if what.startswith("same_next"):
        c = S.pred_case(10, 192, int(what[-1]), 1, same_next=True)
        assert c["sn"] is c["sn_next"]
    else:
        c = S.pred_case(5, 96, 2, 3, bias=what != "no_bias")
    pred, flow, sp, img = _pred_run(c, want_pred=what != "no_pred")
    assert (pred is None) == (what == "no_pred")
    _pred_check(c, pred, flow, sp, img)
    if what == "no_pred":                                      # SN_next(pred) then stands against the float64 prediction: not bit for bit
        p64, _ = S.pred_reference(c, sp)
        got = img[..., c["Cin"] + 32:c["Cin"] + 34].permute(1, 0, 2, 3, 4).float()
        rep = c["sn_next"].report(p64.float().permute(1, 0, 2, 3, 4), got)
        assert rep["unexplained"] == 0, rep


def test_pred_cases_cover_what_they_claim():
    """every class-2 setting at every D, plif on both sides of class 0, every shape, and the shapes' position counts on both sides of a
    workgroup's share"""
    for D in S.PRED_D:
        used = {n.name for Cin in S.PRED_CIN for n in S.pred_neurons(D, Cin, 2)}
        assert used == set(S.CLASS2), (D, used)
        assert {S.pred_neurons(D, Cin, 0)[0].name for Cin in S.PRED_CIN} == {"lif", "plif"}
        if D <= 10:
            a, b = S.pred_neurons(D, 96, 1)
            assert not torch.equal(a.psn_w, b.psn_w)
    assert {_pred_shape(*k) for k in PRED_ALL} == {0, 1, 2, 3}
    assert 1 * 3 * 4 < 4 * (64 // 8) and 2 * 5 * 7 > 2 * 4 * (64 // 8)
    assert any(sy != sx for *_, sy, sx in S.PRED_SHAPES) and {sy for *_, sy, sx in S.PRED_SHAPES} == {1, 2, 16}


# ==================================================================================================== 3. one-launch QK front
class _Lin:
    """a linear layer as 16-bit planes + its BatchNorm"""

    def __init__(self, lin, planes=2):
        self.N, self.K = lin["W"].shape
        self.Wp = hip.split_weight(_dev(lin["W"]), planes)
        self.alpha, self.beta, self.bias = _dev(lin["alpha"]), _dev(lin["beta"]), _dev(lin.get("bias"))


def _weff(Wp):
    """the float64 value of the weight the device's planes carry"""
    if Wp.shape[0] == 2:
        return Wp.cpu().view(torch.float16).double().sum(0) * Wp.sdf_acc_scale
    return Wp.cpu().view(torch.bfloat16).double().sum(0)


QK_CASES = [(cls, Cc, geom, form) for cls in (0, 1, 2) for Cc in (96, 192) for geom in S.QK_GEOM for form in ("separate", "stacked")
            if not (form == "stacked" and cls == 1)]


@gpu
@pytest.mark.parametrize("cls,Cc,geom,form", QK_CASES)
def test_qk_front(monkeypatch, cls, Cc, geom, form):
    """qk_front_kernel<class, KEEP>: against the four-launch form of the entry point (bit-equal) and against the oracle step by step"""
    _route(monkeypatch, SDF_QK_FRONT_ANY="1", SDF_WIDE="0")
    c = S.qk_case(Cc, geom, form, cls)
    B, D, H, W, window, shift = c["geom"]
    Tq, N1, nH, B_, M = c["Tq"], c["N1"], c["nH"], c["B_"], c["Tq"] * c["rows"]
    rowmap, nwin = hip.window_slice_map(B, D, H, W, window, shift, DEV)
    assert nwin == B_ and torch.equal(rowmap.cpu(), c["map"]) and (geom != "w9" or bool((c["map"] < 0).any()))
    p, q_lin, k_lin, pe = _Lin(c["lin"]["p"]), _Lin(c["lin"]["q"]), _Lin(c["lin"]["k"]), _dev(c["pe"])
    if form == "stacked":
        Wp = hip.split_weight(torch.cat([_dev(c["lin"]["q"]["W"]), _dev(c["lin"]["k"]["W"])], 0).contiguous(), 2)
        kw = dict(qk={"Wp": Wp, "alpha": torch.cat([q_lin.alpha, k_lin.alpha]).contiguous(), "beta": torch.cat([q_lin.beta, k_lin.beta]).contiguous(),
                      "add": torch.cat([torch.zeros_like(pe), pe], 1).contiguous()})
        w = _weff(Wp)
        assert torch.equal(w[:Cc], c["held"]["q"]) and torch.equal(w[Cc:], c["held"]["k"])
    else:
        kw = dict(q_lin=q_lin, k_lin=k_lin, pe=pe)
        assert torch.equal(_weff(q_lin.Wp), c["held"]["q"]) and torch.equal(_weff(k_lin.Wp), c["held"]["k"])
    ns = [_np(n) for n in c["sn"]]
    x0 = _dev(c["x"])

    def run(tape, four=False):
        def call():
            keep = [] if tape else None
            y = hip.qk_attn(x0.clone(), rowmap, B_, Tq, N1, nH, p, *ns, keep_ws=keep, four_launches=four, **kw)
            if not tape:
                return (y,)
            ws = keep[0]
            return y, ws[:M * Cc], ws[(M * Cc + 255) // 256 * 256:][:2 * M * Cc]
        return call

    def front(tape):
        outs = []
        for _ in range(2):
            got, out = logged(run(tape))
            assert got[0] == c["route"] % ("true" if tape else "false") and len(got) >= 2, got
            assert all("spike_" in line or "splitk" in line for line in got[1:]), got          # (the projection; nothing else before it)
            outs.append(out)
        assert all(a.data_ptr() != b.data_ptr() and torch.equal(a, b) for a, b in zip(*outs)), "two calls differ"
        return outs[0]
    y, e, qk = front(True)
    (y_plain,) = front(False)
    assert torch.equal(y, y_plain) and not torch.equal(y, x0), "the tape changes the block's output"
    # (a) the four-launch form of the same entry point
    got4, (y4, e4, qk4) = logged(run(True, four=True))
    assert len(got4) >= (4 if form == "stacked" else 5) and not any("qk_front" in line for line in got4), got4
    assert torch.equal(qk, qk4), f"q | k spikes differ from the four-launch form in {int((qk != qk4).sum())} of {qk.numel()} bytes"
    assert torch.equal(e, e4) and torch.equal(y, y4)
    # (b) the oracle, step by step
    q, k = (t.cpu() for t in S.qk_tape(c, qk))
    rq, rk = S.qk_check(c, q, k, e.cpu().view(Tq, c["rows"], Cc))
    for nm, r in (("q", rq), ("k", rk)):
        print(f"\nS0PAR qk_front {c['route'] % 'true'} {nm} n {r['n']} ambiguous {r['ambiguous']} flips {r['flips']} needed {r['needed']:.3e}")


@pytest.mark.parametrize("cls,Cc,geom,form", QK_CASES)
def test_qk_front_premise(cls, Cc, geom, form):
    """the reference's own spikes pass the oracle check; q, k and the slice spikes fire inside (0.03, 0.97), the gate inside (0.1, 0.9);
    the four neurons differ (sn_k is sn_q in the stacked form, by the entry point's contract)"""
    c = S.qk_case(Cc, geom, form, cls)
    for s in (c["sproj"], c["q"], c["k"]):
        S.check_rate(s)
    S.check_rate(c["gate"], 0.1, 0.9)
    sn = c["sn"]
    assert all(n.cls == cls for n in sn)
    pairs = [(a, b) for i, a in enumerate(sn) for b in sn[i + 1:]]
    assert sum(a.same_settings(b) for a, b in pairs) == (1 if form == "stacked" else 0) and (sn[1] is sn[2]) == (form == "stacked")
    e = (c["k"].view(c["Tq"], c["rows"], c["nH"], 32) * c["gate"][..., None]).view(c["Tq"], c["rows"], Cc).to(torch.uint8)
    rq, rk = S.qk_check(c, c["q"].to(torch.uint8), c["k"].to(torch.uint8), e)
    assert rq["flips"] == rk["flips"] == 0 and rq["ambiguous"] <= S.AMBIGUOUS_CAP * rq["n"] and rk["ambiguous"] <= S.AMBIGUOUS_CAP * rk["n"]
    assert 0.03 < float(e.float().mean()) < 0.9


def test_slice_map_restated():
    m, B_ = S.slice_map(1, 4, 11, 13, (2, 9, 9), (1, 4, 4))
    assert B_ == 8 and m.numel() == 8 * 2 * 81
    real = m[m >= 0]
    assert real.numel() == 4 * 11 * 13 and torch.equal(real.sort().values, torch.arange(4 * 11 * 13, dtype=torch.int32))
    m, B_ = S.slice_map(1, 2, 5, 5, (2, 5, 5), (0, 0, 0))
    assert B_ == 1 and torch.equal(m, torch.arange(50, dtype=torch.int32))


# ==================================================================================================== 4. one-launch MS MLP
MLP_CASES = [(2, D, C, 2, 0) for D in (5, 10, 20) for C in (96, 192)] + [(2, 10, C, ns, 0) for C in (96, 192) for ns in (1, 3)] + \
            [(0, D, C, 2, 0) for D in (5, 10, 20) for C in (96, 192)] + [(1, D, C, 2, 0) for D in (5, 10) for C in (96, 192)] + \
            [(cls, 10, C, ns, 0) for cls in (0, 1) for C in (96, 192) for ns in (1, 3)] + \
            [(2, 20, 192, 2, 1), (2, 10, 96, 2, 1), (2, 10, 96, 3, 1), (0, 5, 96, 2, 1), (1, 10, 192, 2, 1)]     # (class, D, C, planes, shape)


@gpu
@pytest.mark.parametrize("cls,D,C,ns,shape", MLP_CASES)
def test_ms_mlp_one_launch(monkeypatch, cls, D, C, ns, shape):
    """ms_mlp_fused_kernel<planes, D, .., class, KEEP> with sn1 != sn2: the three steps against the oracle; tape and no tape give the same x"""
    _route(monkeypatch, SDF_MLP_FUSED_ANY="1")
    c = S.mlp_case(D, C, cls, ns, shape)
    fc1, fc2 = _Lin(c["fc1"], ns), _Lin(c["fc2"], ns)
    assert torch.equal(_weff(fc1.Wp), c["fc1"]["held"]) and torch.equal(_weff(fc2.Wp), c["fc2"]["held"])
    n1, n2, x0 = _np(c["sn1"]), _np(c["sn2"]), _dev(c["x"])
    ntok, Ch = c["ntok"], c["Ch"]
    s2_at = (ntok * C + 255) // 256 * 256

    def run(tape):
        def call():
            ws = hip.ms_mlp_workspace(x0, Ch).fill_(7)
            y = hip.ms_mlp(x0.clone(), fc1, fc2, n1, n2, keep_ws=[] if tape else None, ws=ws)
            return y, ws
        return call
    y, ws = _twice(run(True), [c["route"] % "true"])
    y_plain, ws_plain = _twice(run(False), [c["route"] % "false"])
    assert torch.equal(y, y_plain) and not torch.equal(y, x0), "the tape changes the output"
    assert bool((ws_plain == 7).all()), "without the tape the one-launch form writes nothing but x"
    ws = ws.cpu()
    s1, s2 = ws[:ntok * C].view(ntok, C), ws[s2_at:s2_at + ntok * Ch].view(ntok, Ch)
    assert int(s1.max()) <= 1 and int(s2.max()) <= 1, "a spike of the tape was never written"
    assert bool((ws[ntok * C:s2_at] == 7).all()) and bool((ws[s2_at + ntok * Ch:] == 7).all()), "a store outside the two spike tensors"
    rep = S.mlp_check(c, s1, s2, y.cpu())
    print(f"\nS0PAR mlp {c['route'] % 'true'} n {rep['n']} ambiguous {rep['ambiguous']} flips {rep['flips']} needed {rep['needed']:.3e}")


@pytest.mark.parametrize("cls,D,C,ns,shape", MLP_CASES)
def test_ms_mlp_premise(cls, D, C, ns, shape):
    """sn1 != sn2 in settings, both of the class; on the reference's own spikes the three-step check passes and both neurons fire inside
    (0.03, 0.97); the shapes sit on both sides of a work item's share of positions"""
    c = S.mlp_case(D, C, cls, ns, shape)
    assert c["sn1"].cls == c["sn2"].cls == cls and not c["sn1"].same_settings(c["sn2"])
    S.check_rate(c["s1"])
    s2 = c["sn2"].ref(S.mlp_pre2(c, c["s1"]))
    ref2 = s2.view(D, c["B"], c["H"] * c["W"], c["Ch"]).permute(1, 0, 2, 3).reshape(c["ntok"], c["Ch"]).to(torch.uint8)
    xo = c["x"].reshape(c["ntok"], C).double() + (ref2.double() @ c["fc2"]["held"].t()) * c["fc2"]["alpha"].double() + c["fc2"]["beta"].double()
    rep = S.mlp_check(c, c["s1"], ref2, xo.float())
    assert rep["flips"] == 0 and rep["ambiguous"] <= S.AMBIGUOUS_CAP * rep["n"]
    ppi = S.mlp_geometry(ns, D, C)[0]
    P = c["B"] * c["H"] * c["W"]
    assert P % ppi, "the positions are a whole number of work items"


def test_mlp_cases_cover_what_they_claim():
    for D in (5, 10, 20):
        assert {n.name for C in (96, 192) for n in S.mlp_neurons(2, D, C)} == set(S.CLASS2)
    assert {(cls, D, C) for cls, D, C, ns, _ in MLP_CASES if ns == 2} >= {(2, D, C) for D in (5, 10, 20) for C in (96, 192)}
    for k in (0, 1, 2):
        assert {(C, ns) for cls, D, C, ns, _ in MLP_CASES if cls == k and D == 10} == {(C, ns) for C in (96, 192) for ns in (1, 2, 3)}
    # every <planes, T, width, class> launch_t has (PSN has none at T = 20; one / three planes only at T = 10), each with and without the tape
    assert {(ns, D, C, cls) for cls, D, C, ns, _ in MLP_CASES} == {(ns, D, C, cls) for ns in (1, 2, 3) for D in (5, 10, 20) for C in (96, 192)
                                                                   for cls in (0, 1, 2) if (ns == 2 or D == 10) and not (cls == 1 and D == 20)}


# ==================================================================================================== 5. token gate
@gpu
@pytest.mark.parametrize("layout", ("dense", "stacked"))
@pytest.mark.parametrize("Cc", (32, 96, 192))
@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("Tq", (1, 2, 3, 4))
def test_qk_gate(Tq, name, Cc, layout):
    """qk_gate_kernel on dense q / k and on the halves of one stacked q | k buffer (ldq = ldk = 2 C): e = k AND SN(head sums of q), bit
    for bit, nothing written outside e"""
    c = S.gate_case(Tq, name, Cc)
    rows, g = c["rows"], S.GATE_GUARD
    if layout == "dense":
        q, k, ld = _dev(c["q"]), _dev(c["k"]), None
    else:
        both = _dev(torch.cat([c["q"], c["k"]], 2))
        q, k, ld = both, both.view(-1)[Cc:], 2 * Cc
    bufs = []

    def call():
        buf = torch.full((g + Tq * rows + g, Cc), 7, dtype=torch.uint8, device=DEV)
        bufs.append(buf)
        hip.qk_gate(q, k, buf[g:g + Tq * rows], Tq, rows, Cc, _np(c["sn"]), ldq=ld, ldk=ld)
        return (buf,)
    (buf,) = _twice(call, c["route"])
    buf = buf.cpu()
    assert bool((buf[:g] == 7).all()) and bool((buf[g + Tq * rows:] == 7).all()), "a store outside e"
    assert torch.equal(buf[g:g + Tq * rows].view(Tq, rows, Cc), c["e"])


@pytest.mark.parametrize("Cc", (32, 96, 192))
@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("Tq", (1, 2, 3, 4))
def test_qk_gate_premise(Tq, name, Cc):
    c = S.gate_case(Tq, name, Cc)
    S.check_rate(c["gate"], 0.1, 0.9)
    assert (c["rows"] * (Cc // 32)) % 256 and c["rows"] * (Cc // 32) > 256           # a partial last workgroup behind a full one
