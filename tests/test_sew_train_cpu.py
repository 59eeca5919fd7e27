"""Training of the SEW family (SpikingformerFlowNet), host side: the oracle's TRAIN mode pinned on the real reference by the
spike-forced step record (tests/golden/sew_train_step_forced.npz, make_golden_sew_train.py), the new entry point's ABI (header,
signature table, descriptor mirror, argument refusals before any launch, workspace sizes) and the refusal of CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sdformerflow_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "sew_train_step_forced.npz"))


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_oracle_sew_train_mode_is_pinned_by_the_spike_forced_reference_run(kind):
    """The oracle's TRAIN-mode `forward_sew_flownet` with the reference's spikes forced into all 75 neuron layers (3-encoder model,
    144 x 192, batch 2): both graphs carry identical spike trains, so the loss agrees to 1e-6, every decision the oracle's own
    pre-activation would have taken differently lies within a 16-ulp threshold margin (0 unexplained), and every parameter gradient
    is within 5e-5 of the reference's largest element.  The GPU side of the same statement: tests/test_sew_train_gpu.py."""
    lr, lo = (float(v) for v in FIX[f"{kind}_loss"])
    assert abs(lr - lo) <= 1e-6 * abs(lr), (lr, lo)
    fun = FIX[f"{kind}_flips_unexplained_n"]
    assert len(fun) == 75 and int(fun[:, 1].sum()) == 0
    assert int(fun[:, 0].sum()) <= 1e-6 * int(fun[:, 2].sum())
    rel = FIX[f"{kind}_grad_rel"]
    live = rel[rel >= 0]
    assert len(live) >= 150 and float(live.max()) <= 5e-5, float(live.max())
    names = [str(n) for n in FIX[f"{kind}_grad_names"]]
    assert any(n.endswith("relative_position_bias_table") and r >= 0 for n, r in zip(names, rel))


def test_parameter_names_match_the_reference():
    import yaml
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    for kind in ("lif", "psn"):
        cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
        cfg["swin_transformer"].update(input_size=[144, 192], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
        m = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
        assert [n for n, _ in m.named_parameters()] == [str(n) for n in FIX[f"{kind}_grad_names"]]


def test_binding_matches_the_header_for_the_sew_backward():
    src = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    assert re.search(r"^int64_t sdf_win_attn_sew_bwd_workspace_bytes\(int B_, int nH, int N\);", src, flags=re.M)
    assert re.search(r"^int sdf_win_attn_sew_bwd\(const SdfWinAttnSewBwdDesc\* d, void\* stream\);", src, flags=re.M)
    assert hip.SIGNATURES["sdf_win_attn_sew_bwd_workspace_bytes"] == (C.c_int64, (C.c_int, C.c_int, C.c_int))
    assert hip.SIGNATURES["sdf_win_attn_sew_bwd"] == (C.c_int, (C.POINTER(hip.WinAttnSewBwdDesc), C.c_void_p))
    body = re.search(r"typedef struct SdfWinAttnSewBwdDesc \{(.*?)\} SdfWinAttnSewBwdDesc;", src, flags=re.S).group(1)
    members = re.findall(r"(\w+)(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f for f, _ in hip.WinAttnSewBwdDesc._fields_] == members


def _desc(**kw):
    d = hip.WinAttnSewBwdDesc()
    for f in ("q", "k", "v", "dout", "scale", "bias", "dq", "dk", "dv", "d_bias", "workspace"):
        setattr(d, f, 0x10000)                                  # never dereferenced: every case is refused before a launch
    d.workspace_bytes = 1 << 40
    d.B_, d.nW, d.nH, d.Tq, d.N1, d.hd = 4, 1, 3, 2, 81, 32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_sew_backward_refusals_and_workspace():
    lib = hip.lib()
    f = lib.sdf_win_attn_sew_bwd
    assert f(None, None) == hip.E_NULL
    assert f(C.byref(_desc(dout=None)), None) == hip.E_NULL
    assert f(C.byref(_desc(workspace=None)), None) == hip.E_NULL
    assert f(C.byref(_desc(hd=16)), None) == hip.E_SHAPE
    assert f(C.byref(_desc(N1=97)), None) == hip.E_SHAPE                              # N = 194 > 192
    assert f(C.byref(_desc(Tq=0)), None) == hip.E_SHAPE
    assert f(C.byref(_desc(nH=0)), None) == hip.E_SHAPE
    assert f(C.byref(_desc(mask=0x10000, nW=3)), None) == hip.E_SHAPE                # B_ % nW != 0
    assert f(C.byref(_desc(workspace_bytes=1024)), None) == hip.E_SHAPE              # workspace too small
    assert f(C.byref(_desc(dout=0x10004)), None) == hip.E_ALIGN
    wb = lib.sdf_win_attn_sew_bwd_workspace_bytes
    assert wb(4, 3, 193) == 0 and wb(0, 3, 162) == 0
    # split-K partials: runs x nH x N x N fp32 - runs as the kernel plans them, never a slab per window
    assert wb(4, 3, 162) == -(-4 * 3 * 162 * 162 * 4 // 256) * 256
    assert 0 < wb(1760, 3, 162) <= 64 * 3 * 162 * 162 * 4 + 256


def test_cpu_tensors_are_refused():
    q = torch.zeros((2, 1, 81, 96), dtype=torch.uint8)
    with pytest.raises(hip.SdfError):
        hip.win_attn_sew_bwd(q, q, q, torch.ones(3), torch.zeros((3, 162, 162)), None, 3, 2, 1, 81, torch.zeros((2, 1, 81, 96)))
    from sdformerflow_amd import train
    with pytest.raises(hip.SdfError):
        train.forward_train_sew(None, torch.zeros((1, 10, 2, 16, 16)))


def test_the_attention_module_refuses_training_at_module_level():
    from sdformerflow_amd.STSwinNet_SNN.Spiking_swin_transformer3D import Spiking_BN_WindowAttention3D
    attn = Spiking_BN_WindowAttention3D(96, (2, 9, 9), (0, 0, 0), 3, norm="BN", num_steps=2, v_reset=None, v_th=0.1, neuron_type="lif",
                                        surrogate_fun="surrogate.ATan()", tau=2.0, detach_reset=True, spike_norm="BN").train()
    with pytest.raises(NotImplementedError, match="forward_train_sew"):
        attn(torch.zeros((2, 1, 9, 9, 96)))


def test_torch_core_equals_the_oracle_core():
    """The SDF_SEW_ATTN_BWD=0 composition is the oracle's core (fp64, masked, per-head scale)."""
    from oracle import sdformer_oracle as O
    from sdformerflow_amd import train
    g = torch.Generator().manual_seed(5)
    Tq, B_, N1, nH = 2, 6, 81, 3
    q, k, v = ((torch.rand((Tq, B_, N1, 96), generator=g) < 0.3).double() for _ in range(3))
    bias = torch.randn((nH, 162, 162), generator=g, dtype=torch.float64)
    mask = torch.where(torch.rand((3, 162, 162), generator=g) < 0.5, -100.0, 0.0).double()
    got = train.sew_attention_core_torch(q, k, v, torch.full((nH,), 0.125, dtype=torch.float64), bias, mask, nH)
    want, _ = O.sew_attention_core(*(t.reshape(B_, nH, 162, 32) for t in (q, k, v)), 0.125, bias, mask, Tq, N1)
    assert (got.double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()     # (the composition runs in fp32)
