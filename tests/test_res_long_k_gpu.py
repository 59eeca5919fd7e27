"""K above 1 024 on the weight-resident row-loop kernels (csrc/ms_res.hip): fc2 of the 384-channel stage (K = 1 536) with the fp32
epilogue and, in the lean build, with the emitted neuron, and the merge of 384 channels (K = 4 C = 1 536) - through the C ABI
(hip.ms_mlp, hip.ms_patch_merge).

Every case runs twice: as routed (SDF_RES_LONGK_UNITS=1 lifts the row bound under which the K ring keeps such a launch, so that the
small shapes here reach the row loop) and with SDF_RES_MAXK=1024 - the K-ring route, the routing before these forms.  The two are
bit-equal (exact integer sums, the same fp32 epilogue expressions), the launch log names the kernel family each leg ran, and the result
is held to the fp64 reference the way tests/test_ms_wide_gpu.py does (fc2: 1e-5 of the output's range on the kernels' own hidden spikes;
merge: 1e-6; emitted spikes: bit-equal to the oracle neuron on the kernel's own updated x).

What does not fit a compute unit's LDS whole (K = 3 072: 288 KB of digits per 32 columns) stays on the K ring under either setting: its
case holds the routing to that and the result to the same reference."""
import pytest
import torch

import routes_common
from sdformerflow_amd import hip
from sdformerflow_amd.synthetic import synth_uniform as rnd
from test_ms_wide_gpu import _L, _N, _merge_ref, _weff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LONG = {"SDF_RES_LONGK_UNITS": "1"}
RING = {"SDF_RES_LONGK_UNITS": "1", "SDF_RES_MAXK": "1024"}


def _last_kernel(lines):
    return lines[-1].split(" ", 3)[3]


def _mlp_case(B, D, H, W, Cc, Ch, seed):
    x0 = rnd((B, D, H, W, Cc), seed, -0.5, 1.0)
    W1, W2 = rnd((Ch, Cc), seed + 1, -0.15, 0.15), rnd((Cc, Ch), seed + 2, -0.05, 0.05)
    fc1 = _L(W1, rnd((Ch,), seed + 3, 0.5, 1.5), rnd((Ch,), seed + 4, -0.2, 0.2))
    fc2 = _L(W2, rnd((Cc,), seed + 5, 0.5, 1.5), rnd((Cc,), seed + 6, -0.2, 0.2))
    if hasattr(fc2, "digits_tiled"):
        del fc2.digits_tiled                                        # (fc2 through launch_pm, not on the small-M kernel)
    return x0, fc1, fc2


def _fc2_reference(x0, fc1, fc2, n1, n2):
    """x + BN2(s2 W2^T) in fp64 on the kernels' own hidden spikes: the parity tape of a call of its own (fc1 is the same launch on
    every route, the tape only changes the hand-over layout)"""
    B, D, H, W, Cc = x0.shape
    ntok, Ch = B * D * H * W, fc1.N
    keep = []
    with hip.scoped_switches(**RING):
        hip.ms_mlp(x0.to(DEV).clone(), fc1, fc2, n1.p, n2.p, keep_ws=keep)
    torch.cuda.synchronize()
    s2 = keep[0].cpu()[(ntok * Cc + 255) // 256 * 256:][:ntok * Ch].view(ntok, Ch)
    assert 0.03 < s2.float().mean() < 0.97
    return x0.reshape(ntok, Cc).double() + (s2.double() @ _weff(fc2.digits).t()) * fc2.alpha.cpu().double() + fc2.beta.cpu().double()


def _run_mlp(x0, fc1, fc2, n1, n2, emit, env):
    buf = torch.full(x0.shape, 7, dtype=torch.uint8, device=DEV) if emit is not None else None
    with hip.scoped_switches(**env):
        lines, x = routes_common.logged(lambda: hip.ms_mlp(x0.to(DEV).clone(), fc1, fc2, n1.p, n2.p,
                                                           emit_next=None if emit is None else (buf, emit.p)))
    return _last_kernel(lines), x, buf


def _check_fc2(B, D, H, W, Cc, Ch, block, emit_name, want, seed):
    x0, fc1, fc2 = _mlp_case(B, D, H, W, Cc, Ch, seed)
    n1, n2 = _N(block, D, seed=1), _N(block, D, seed=2)
    emit = None if emit_name is None else _N(emit_name, D, v_th=0.25, seed=21, bias=-0.2)
    ka, xa, ba = _run_mlp(x0, fc1, fc2, n1, n2, emit, LONG)
    kb, xb, bb = _run_mlp(x0, fc1, fc2, n1, n2, emit, RING)
    assert ka.startswith(want) and kb.startswith("wide_pm_kernel<"), (ka, kb)
    assert torch.equal(xa, xb), "x differs between the row loop and the K ring"
    ref = _fc2_reference(x0, fc1, fc2, n1, n2)
    err = (xa.cpu().reshape(ref.shape).double() - ref).abs().max().item()
    print(f"\nLONGK {ka} err/range {err / ref.abs().max().item():.2e}")
    assert err <= 1e-5 * ref.abs().max().item(), err
    if emit is not None:
        assert torch.equal(ba, bb), "the emitted spikes differ between the row loop and the K ring"
        want_s = emit.ref(xa.cpu().permute(1, 0, 2, 3, 4).contiguous()).permute(1, 0, 2, 3, 4)
        assert torch.equal(ba.cpu().float(), want_s), "emitted spikes differ from the oracle neuron on the updated x"
        assert 0.02 < want_s.mean() < 0.98


# 14 positions at T = 10: one full 8-position unit and a ragged one, the batch boundary inside the first; 5 positions at T = 20: a
# full 4-position unit and a ragged one
@pytest.mark.parametrize("B,D,H,W", [(2, 10, 1, 7), (1, 20, 1, 5)])
def test_fc2_k1536_fp32_epilogue(B, D, H, W):
    _check_fc2(B, D, H, W, 384, 1536, "lif", None, f"res_pm_kernel<{D}, 2, 0, 0, false, false>", 7100)


# the hidden widths ms_wide_mlp_supports admits between 1 024 and 1 536 (multiples of 192): K = 1 152 is 18 64-deep steps, K = 1 344 is
# 21 - an odd count: the main loop's single-step tail
@pytest.mark.parametrize("Ch,D", [(1152, 10), (1344, 10), (1344, 20)])
def test_fc2_hidden_widths_between_1024_and_1536(Ch, D):
    _check_fc2(1, D, 3, 3, 256, Ch, "lif", None, f"res_pm_kernel<{D}, 2, 0, 0, false, false>", 7200)
    _check_fc2(1, D, 3, 3, 256, Ch, "lif", "lif", f"res_pm_lean_kernel<{D}, 0>", 7300)


# the emitted neuron (lean build: the spike bytes leave the transposed quads straight for the row-major output); the class-1 neuron
# (PSN) of the block's own class and the general class 2 (hard reset) emitted from a LIF block
@pytest.mark.parametrize("B,D,H,W,block,emit,nk", [(2, 10, 1, 7, "lif", "lif", 0), (1, 20, 1, 5, "lif", "lif", 0), (2, 10, 1, 7, "psn", "psn", 1),
                                                   (1, 20, 1, 5, "psn", "psn", 1), (2, 10, 1, 7, "lif", "lif_hard", 2)])
def test_fc2_k1536_emits_the_next_neuron(B, D, H, W, block, emit, nk):
    _check_fc2(B, D, H, W, 384, 1536, block, emit, f"res_pm_lean_kernel<{D}, {nk}>", 7400)


@pytest.mark.parametrize("emit", [None, "lif"])
def test_fc2_k3072_keeps_the_k_ring(emit):
    """C = 768 / Ch = 3 072 on a 3 x 3 map: no form of it fits beside 288 KB of digits"""
    _check_fc2(1, 10, 3, 3, 768, 3072, "lif", emit, "wide_pm_kernel<10, 2, 3, 0, 0>" if emit else "wide_pm_kernel<10, 2, 2, 0, 0>", 7500)


# odd maps: 5 x 7 -> 3 x 4 merged positions with zero padding on both edges; C = 320 (K = 1 280) beside the shipped 384
@pytest.mark.parametrize("B,D,H,W,Cc", [(1, 10, 5, 7, 384), (1, 20, 5, 7, 384), (2, 10, 5, 7, 320)])
def test_merge_beyond_256_channels(B, D, H, W, Cc):
    N = 2 * Cc
    sp = (rnd((B, D, H, W, Cc), 7600, 0.0, 1.0) < 0.3).to(torch.uint8)
    lin = _L(rnd((N, 4 * Cc), 7601, -0.08, 0.08), rnd((N,), 7602, 0.5, 1.5), rnd((N,), 7603, -0.2, 0.2))
    with hip.scoped_switches(**LONG):
        la, oa = routes_common.logged(lambda: hip.ms_patch_merge(sp.to(DEV), lin))
    with hip.scoped_switches(**RING):
        lb, ob = routes_common.logged(lambda: hip.ms_patch_merge(sp.to(DEV), lin))
    ka, kb = _last_kernel(la), _last_kernel(lb)
    assert ka == f"res_pm_kernel<{D}, 2, 0, 2, false, false>" and kb == f"wide_pm_kernel<{D}, 2, 2, 0, 2>", (ka, kb)
    assert torch.equal(oa, ob), "the merge differs between the row loop and the K ring"
    ref = _merge_ref(sp, _weff(lin.digits), lin.alpha.cpu(), lin.beta.cpu())
    err = (oa.cpu().double() - ref).abs().max().item()
    print(f"\nLONGK {ka} err/range {err / ref.abs().max().item():.2e}")
    assert err <= 1e-6 * ref.abs().max().item(), err


def test_the_row_bound_of_the_default_routing():
    """Without any switch a launch with K > 1 024 takes the row loop from 64 80-row units on (the size of several samples in one launch
    sequence); below - a single sample's launches - the K ring keeps it: 16 x 32 = 512 positions are 64 units, 21 x 24 = 504 are 63"""
    n1, n2 = _N("lif", 10, seed=1), _N("lif", 10, seed=2)
    for (H, W), want in (((16, 32), "res_pm_kernel<10, 2, 0, 0, false, false>"), ((21, 24), "wide_pm_kernel<10, 2, 2, 0, 0>")):
        x0, fc1, fc2 = _mlp_case(1, 10, H, W, 384, 1536, 7700)
        k, x, _ = _run_mlp(x0, fc1, fc2, n1, n2, None, {})
        assert k == want, (H, W, k)
        _, xr, _ = _run_mlp(x0, fc1, fc2, n1, n2, None, RING)
        assert torch.equal(x, xr)
