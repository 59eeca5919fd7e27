"""Launches of the int8 digit-plane product kernels, pinned kernel by kernel: direct calls of hip.ms_mlp, hip.qk_attn, hip.ms_patch_merge,
hip.spike_conv2d (small-M form), hip.spike_gemm (both digit layouts) and hip.spike_deconv3x3s2 at the smallest shapes their rules admit,
each asserting through hip.launch_log() the LITERAL list of launches - workgroups, threads, dynamic LDS bytes, kernel with its template
arguments - that the library made before the host plans, grid rules and template dispatch of these kernels were stated once
(csrc/host_launch.h).  Recorded on an MI355X.  Together the cases reach res_pm_kernel<T, EPI, NK, AM, small-K, STRIP> with epilogues
1 / 2 / 3, AM 0 / 2 / 3, small-K and strip on and off; res_front_kernel with and without the q | k tape; wide_pm_kernel with 2 and 3
column blocks and epilogues 1 / 2 / 3 (and its patch-merging form); wide_front_kernel with two row blocks; the small-M kernel as
convolution, fc2 and plain product; T = 10 and 20; the neuron classes 0 (LIF, soft reset), 1 (PSN) and 2 (hard reset / IF).

No numeric comparison: parity is covered by test_ms_wide_gpu.py, test_smallm_gpu.py and the route tests.  Outputs go to fresh buffers."""
import pytest
import torch

import routes_common
from routes_common import DEV, neuron, rnd
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
SWITCHES = ("SDF_RES", "SDF_RES_MINC", "SDF_RES_MAXC", "SDF_RES_UPW", "SDF_RES_RMUL", "SDF_RES_STRIP", "SDF_WIDE", "SDF_WIDE_CB",
            "SDF_WIDE_PASSES", "SDF_WIDE_MAXROWS", "SDF_WIDE_CONV", "SDF_SMALLM", "SDF_SMALLM_FC2", "SDF_SMALLM_CB", "SDF_SMALLM_CONV_ROWS")


def spikes(shape):
    return (torch.rand(shape, device=DEV) < 0.3).to(torch.uint8)


class _L:
    def __init__(self, N, K, bias=False, tiled=False):
        W = rnd((N, K))
        self.N, self.K = N, K
        self.Wp = hip.split_weight(W, 2)
        self.digits = hip.split_weight_i8x3(W)
        if tiled:
            self.digits_tiled = hip.tile_weight_i8x3(self.digits)
        self.alpha, self.beta = rnd((N,), 0.5, 1.5), rnd((N,), -0.2, 0.2)
        self.bias = rnd((N,)) if bias else None


def logged(call):
    return routes_common.logged(call)[0]


# ------------------------------------------------------------------------------------------------------------------ the calls
def mlp(Cc, D, HW, name, tape=False, emit=False, tiled=False, B=1):
    Ch = 4 * Cc
    fc1, fc2, n = _L(Ch, Cc), _L(Cc, Ch, tiled=tiled), neuron(name, D)
    x = rnd((B, D, HW[0], HW[1], Cc), -0.5, 1.0)
    kw = {}
    if tape:
        kw["keep_ws"] = []
    if emit:
        kw["emit_next"] = (torch.zeros((B, D, HW[0], HW[1], Cc), dtype=torch.uint8, device=DEV), n)
    return lambda: hip.ms_mlp(x, fc1, fc2, n, n, **kw)


def attn(Cc, D, HW, window, name, tape=False, emit=False, stacked=True):
    nH, Tq, N1 = Cc // 32, window[0], window[1] * window[2]
    x = rnd((1, D, HW[0], HW[1], Cc), -0.5, 1.0)
    plin = _L(Cc, Cc, bias=True)
    if stacked:
        wcat = rnd((2 * Cc, Cc))
        kw = dict(qk={"Wp": hip.split_weight(wcat, 2), "digits": hip.split_weight_i8x3(wcat), "alpha": rnd((2 * Cc,), 0.5, 1.5),
                      "beta": rnd((2 * Cc,), -0.1, 0.3), "add": rnd((Tq * N1, 2 * Cc))})
    else:
        kw = dict(q_lin=_L(Cc, Cc), k_lin=_L(Cc, Cc), pe=rnd((Tq * N1, Cc)))
    rowmap, B_ = hip.window_slice_map(1, D, HW[0], HW[1], window, (0, 0, 0), DEV)
    zsrc = hip.window_zsrc_map(rowmap, B_, Tq, N1, nH, x.numel() // Cc)
    n, ne = neuron(name, Tq), neuron(name, D)
    if tape:
        kw["keep_ws"] = []
    if emit:
        # (without the tape the emitted spikes leave in the tiled hand-over layout, (x_rows + 80) * C bytes: the MLP's workspace holds it)
        kw.update(emit=(hip.ms_mlp_workspace(x, 4 * Cc), ne), info={})
    torch.cuda.synchronize()
    return lambda: hip.qk_attn(x, rowmap, B_, Tq, N1, nH, plin, n, n, n, n, x_src=zsrc, **kw)


def merge(Cc, D, HW, B=1):
    lin, sp = _L(2 * Cc, 4 * Cc), spikes((B, D, HW[0], HW[1], Cc))

    def call():
        assert hip.ms_patch_merge(sp, lin) is not None
    return call


def conv(imgs, HW, Cin, N, T, name=None, tiled=False, membrane=False):
    H, W = HW
    Wp = hip.pack_conv_weight_i8x3(rnd((N, Cin, 3, 3)), tiled=tiled)
    x, rows = spikes((imgs, H, W, Cin)), imgs * H * W
    out = torch.empty((rows, N), dtype=torch.float32, device=DEV) if name is None or membrane else None
    kw = {}
    if name is not None:
        kw = dict(out_spike=torch.empty((rows, N), dtype=torch.uint8, device=DEV), sn=neuron(name, T), sn_T=T,
                  pos=(rows // T, H * W, T * H * W, H * W))
    return lambda: hip.spike_conv2d(x, Wp, imgs, H, W, Cin, H, W, 3, 3, 1, (-1, 0, 1), (-1, 0, 1), out=out, alpha=rnd((N,), 0.5, 1.5),
                                    beta=rnd((N,), -0.2, 0.2), **kw)


def gemm(M, N, K, tiled):
    dg = hip.split_weight_i8x3(rnd((N, K)))
    dg = hip.tile_weight_i8x3(dg) if tiled else dg
    A, out = spikes((M, K)), torch.empty((M, N), dtype=torch.float32, device=DEV)
    return lambda: hip.spike_gemm(A, dg, out, M, N, K, alpha=rnd((N,), 0.5, 1.5), beta=rnd((N,), -0.2, 0.2))


def deconv(imgs, T, HW, Cin, Cout):
    planes = hip.pack_deconv2x2_weight(rnd((Cin, Cout, 3, 3)), Cin)
    s = spikes((imgs, HW[0], HW[1], Cin))
    return lambda: hip.spike_deconv3x3s2(s, planes, imgs, T, HW[0], HW[1], Cin, Cout, alpha=rnd((Cout,), 0.5, 1.5), beta=rnd((Cout,), -0.2, 0.2))


KRING = {"SDF_RES_MAXC": "191"}      # the K-ring kernels (ms_wide.hip) from 192 channels on: the row loop below 192 only
# name: (switches, the call, the launches recorded before the refactor: "workgroups threads LDS-bytes kernel<template arguments>")
CASES = {
    # ---- weight-resident row loop (ms_res.hip): C = 192, Ch = 768; fc1 is a small-K build (K <= 256), fc2 is not
    "mlp_res_lif": ({}, lambda: mlp(192, 10, (5, 7), "lif"), [
        "7 256 0 neuron_kernel<10>",
        "24 512 52224 res_pm_kernel<10, 1, 0, 0, true, false>",
        "8 512 117760 res_pm_kernel<10, 2, 0, 0, false, false>"]),
    "mlp_res_psn_T20_emit_tape": ({}, lambda: mlp(192, 20, (5, 7), "psn", tape=True, emit=True), [
        "7 256 0 neuron_kernel<20>",
        "48 512 53904 res_pm_kernel<20, 1, 1, 0, true, false>",
        "16 512 109200 res_pm_kernel<20, 3, 1, 0, false, false>"]),
    "mlp_res_hard_tape": ({}, lambda: mlp(192, 10, (5, 7), "lif_hard", tape=True), [
        "7 256 0 neuron_kernel<10>",
        "24 512 52224 res_pm_kernel<10, 1, 2, 0, true, false>",
        "8 512 117760 res_pm_kernel<10, 2, 0, 0, false, true>"]),         # (row-major hidden spikes: the strip build)
    "mlp_res384_if_emit_smallm_fc2": ({}, lambda: mlp(384, 10, (5, 7), "if", emit=True, tiled=True), [
        "14 256 0 neuron_kernel<10>",
        "48 512 70656 res_pm_kernel<10, 1, 2, 0, false, false>",
        "64 256 0 smallm_kernel<10, 3, 2, 0, true, 2>"]),
    "mlp_res384_lif_T20_smallm_fc2": ({}, lambda: mlp(384, 20, (3, 3), "lif", tiled=True), [
        "4 256 0 neuron_kernel<20>",
        "48 512 70656 res_pm_kernel<20, 1, 0, 0, false, false>",
        "40 256 0 smallm_kernel<20, 2, 0, 0, true, 2>"]),
    # ---- K ring (ms_wide.hip): C = 384, Ch = 1536; three column blocks once fc1 has >= 600 waves, two below
    "mlp_wide_lif_cb3": (KRING, lambda: mlp(384, 10, (12, 16), "lif"), [
        "72 256 0 neuron_kernel<10>",
        "192 256 0 wide_pm_kernel<10, 3, 1, 0, 0>",
        "72 256 0 wide_pm_kernel<10, 2, 2, 0, 0>"]),
    "mlp_wide_psn_T20_cb2_emit": (KRING, lambda: mlp(384, 20, (5, 7), "psn", emit=True), [
        "14 256 0 neuron_kernel<20>",
        "144 256 0 wide_pm_kernel<20, 2, 1, 1, 0>",
        "40 256 0 wide_pm_kernel<20, 2, 3, 1, 0>"]),
    "mlp_wide_hard_cb2_emit": (KRING, lambda: mlp(384, 10, (5, 7), "lif_hard", emit=True), [
        "14 256 0 neuron_kernel<10>",
        "96 256 0 wide_pm_kernel<10, 2, 1, 2, 0>",
        "24 256 0 wide_pm_kernel<10, 2, 3, 2, 0>"]),
    "mlp_default384_lif": ({}, lambda: mlp(384, 10, (5, 7), "lif"), [
        "14 256 0 neuron_kernel<10>",
        "48 512 70656 res_pm_kernel<10, 1, 0, 0, false, false>",
        "24 256 0 wide_pm_kernel<10, 2, 2, 0, 0>"]),                          # (fc1 on the row loop, fc2 - K = 1536 - on the K ring)
    # ---- attention: N1 = 25 >= 24, Tq = 2
    "attn_res_lif_tape_emit": ({}, lambda: attn(192, 10, (5, 5), (2, 5, 5), "lif", tape=True, emit=True), [
        "24 256 0 neuron_kernel<2>",
        "8 512 65536 res_front_kernel<0, true>",
        "8 512 52224 res_pm_kernel<10, 3, 0, 0, true, false>"]),
    "attn_res_psn_T20": ({}, lambda: attn(192, 20, (5, 5), (2, 5, 5), "psn", stacked=False), [
        "47 256 0 neuron_kernel<2>",
        "16 512 49152 res_front_kernel<1, false>",
        "8 512 62464 res_pm_kernel<20, 2, 0, 0, true, false>"]),
    "attn_res_if_emit": ({}, lambda: attn(192, 10, (5, 5), (2, 5, 5), "if", emit=True), [
        "24 256 0 neuron_kernel<2>",
        "8 512 49152 res_front_kernel<2, false>",
        "8 512 52224 res_pm_kernel<10, 3, 2, 0, true, false>"]),
    "attn_wide_lif_tape": (KRING, lambda: attn(384, 10, (5, 5), (2, 5, 5), "lif", tape=True), [
        "47 256 0 neuron_kernel<2>",
        "24 256 0 wide_front_kernel<2, 0, true>",
        "16 256 0 wide_pm_kernel<10, 2, 2, 0, 0>"]),
    "attn_wide_hard_T20_emit": (KRING, lambda: attn(384, 20, (5, 5), (2, 5, 5), "lif_hard", emit=True), [
        "94 256 0 neuron_kernel<2>",
        "48 256 0 wide_front_kernel<2, 2, false>",
        "24 256 0 wide_pm_kernel<20, 2, 3, 2, 0>"]),
    "attn_wide_psn_emit": (KRING, lambda: attn(384, 10, (5, 5), (2, 5, 5), "psn", emit=True, stacked=False), [
        "47 256 0 neuron_kernel<2>",
        "24 256 0 wide_front_kernel<2, 1, false>",
        "16 256 0 wide_pm_kernel<10, 2, 3, 1, 0>"]),
    # ---- patch merging: the row loop up to 256 channels (K = 4 C; small-K at C = 64), the K ring beyond
    "merge_res_c64_T20": ({}, lambda: merge(64, 20, (5, 7)), [
        "8 512 68608 res_pm_kernel<20, 2, 0, 2, true, true>"]),
    "merge_res_c96": ({}, lambda: merge(96, 10, (5, 7), B=2), [
        "8 512 80896 res_pm_kernel<10, 2, 0, 2, false, true>"]),
    "merge_wide_c320": ({}, lambda: merge(320, 10, (5, 7)), [
        "24 256 0 wide_pm_kernel<10, 2, 2, 0, 2>"]),
    # ---- small-M kernel: convolution (row-major and fragment-order digits), plain product
    "conv_smallm_f32": ({}, lambda: conv(10, (5, 7), 64, 64, 10), [
        "16 256 0 smallm_kernel<10, 2, 0, 1, false, 2>"]),
    "conv_smallm_tiled_psn_T20": ({}, lambda: conv(20, (5, 7), 64, 96, 20, "psn", tiled=True), [
        "32 256 0 smallm_kernel<20, 1, 1, 1, true, 2>"]),
    "conv_smallm_tiled_hard_membrane": ({}, lambda: conv(10, (5, 7), 128, 64, 10, "lif_hard", tiled=True, membrane=True), [
        "16 256 0 smallm_kernel<10, 3, 2, 1, true, 2>"]),
    "conv_smallm_lif": ({}, lambda: conv(10, (5, 7), 64, 64, 10, "lif"), [
        "16 256 0 smallm_kernel<10, 1, 0, 1, false, 2>"]),
    "gemm_tiled": ({}, lambda: gemm(350, 96, 128, True), [
        "16 256 0 smallm_kernel<10, 2, 0, 0, true, 2>"]),
    # ---- plain product and 2 x 2 transposed convolution on the row loop
    "gemm_rowmajor_k128": ({}, lambda: gemm(350, 96, 128, False), [
        "8 512 56320 res_pm_kernel<10, 2, 0, 0, true, true>"]),
    "gemm_rowmajor_k384": ({}, lambda: gemm(350, 96, 384, False), [
        "8 512 80896 res_pm_kernel<10, 2, 0, 0, false, true>"]),
    "deconv_c64": ({}, lambda: deconv(10, 10, (5, 7), 64, 32), [
        "8 512 68608 res_pm_kernel<10, 2, 0, 3, true, true>"]),
    "deconv_c96_T20": ({}, lambda: deconv(20, 20, (5, 7), 96, 8), [
        "8 512 80896 res_pm_kernel<20, 2, 0, 3, false, true>"]),
}


def launches(name, monkeypatch):
    env, make, _ = CASES[name]
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(0)
    call = make()
    torch.cuda.synchronize()
    return logged(call)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_are_those_recorded(name, monkeypatch):
    got = launches(name, monkeypatch)
    print(name, got)
    assert got == CASES[name][2]


def test_the_cases_reach_every_route():
    """The table itself: what the issue of this test asks the cases to reach, read off the recorded kernel names."""
    seen = {line.split(" ", 3)[3] for _, _, want in CASES.values() for line in want}
    args = lambda kernel: [tuple(a.strip() for a in s[len(kernel) + 1:-1].split(",")) for s in seen if s.startswith(kernel + "<")]
    res, wide, small = args("res_pm_kernel"), args("wide_pm_kernel"), args("smallm_kernel")
    assert {a[1] for a in res} == {"1", "2", "3"} and {a[3] for a in res} == {"0", "2", "3"}
    assert {a[4] for a in res} == {"true", "false"} and {a[5] for a in res} == {"true", "false"}
    assert {a[1] for a in args("res_front_kernel")} == {"true", "false"}
    assert {a[1] for a in wide} == {"2", "3"} and {a[2] for a in wide} == {"1", "2", "3"} and any(len(a) == 5 and a[4] == "2" for a in wide)
    assert any(a[0] == "2" for a in args("wide_front_kernel"))
    assert {a[3] for a in small} == {"0", "1"} and {a[4] for a in small} == {"true", "false"}
    for fam in (res, wide, small):
        assert {a[0] for a in fam} == {"10", "20"}
    assert {a[2] for a in res} == {a[3] for a in wide} == {a[2] for a in small} == {"0", "1", "2"}
