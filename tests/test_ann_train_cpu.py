"""Training of the ANN STTFlowNet, host side: the attention backward entry points' argument refusals and workspace sizes (no
launch), the stochastic-depth schedule of the STT_voxel model and the unchanged state_dict schema."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F
import yaml

from sdformerflow_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(size=(144, 192)):
    from sdformerflow_amd.STSwinNet import STSwinNet
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")))
    return STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), dict(cfg["swin_transformer"], input_size=list(size)))


def _desc(**kw):
    d = hip.WinAttnBwdDesc()
    for f in ("qkv", "pad_qkv", "dout", "scale", "bias", "dqkv", "d_pad", "d_scale", "d_bias", "workspace"):
        setattr(d, f, 0x10000)                                  # never dereferenced: every case is refused before a launch
    d.workspace_bytes = 1 << 40
    d.B_, d.nW, d.nH, d.N, d.hd = 4, 1, 3, 162, 32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_attention_backward_refusals():
    lib = hip.lib()
    assert lib.sdf_win_attn_ann_bwd(None, None) == hip.E_NULL
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(dout=None)), None) == hip.E_NULL
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(workspace=None)), None) == hip.E_NULL
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(row_map=0x10000, d_pad=None)), None) == hip.E_NULL
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(hd=16)), None) == hip.E_SHAPE
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(N=193)), None) == hip.E_SHAPE
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(nH=0)), None) == hip.E_SHAPE
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(mask=0x10000, nW=3)), None) == hip.E_SHAPE       # B_ % nW != 0
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(workspace_bytes=1024)), None) == hip.E_SHAPE     # workspace too small
    assert lib.sdf_win_attn_ann_bwd(C.byref(_desc(qkv=0x10004)), None) == hip.E_ALIGN


def test_attention_backward_workspace_bytes():
    wb = hip.lib().sdf_win_attn_ann_bwd_workspace_bytes
    # (B_, nH, NP, NP) dS slabs + (B_, nH) d_scale partials + (B_, nH, 96) d_pad partials, each rounded up to 256 bytes
    assert wb(C.c_int(4), C.c_int(3), C.c_int(162)) == 4 * 3 * 176 * 176 * 4 + 256 + 4 * 3 * 96 * 4
    assert wb(C.c_int(1), C.c_int(1), C.c_int(98)) == 112 * 112 * 4 + 256 + 512
    assert wb(C.c_int(704), C.c_int(3), C.c_int(162)) == 704 * 3 * 176 * 176 * 4 + 8448 + 704 * 3 * 96 * 4
    assert wb(C.c_int(4), C.c_int(3), C.c_int(193)) == 0
    assert wb(C.c_int(0), C.c_int(3), C.c_int(162)) == 0


def test_drop_path_schedule_of_the_stt_voxel_model():
    from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import SwinTransformerBlock3D
    blocks = [m for m in build().modules() if isinstance(m, SwinTransformerBlock3D)]
    assert len(blocks) == 10
    want = torch.linspace(0, 0.2, 10).tolist()                  # reference swin_transformer3D_v2.py:611, STSwinNet.py:95
    assert [b.drop_path for b in blocks] == want


def test_state_dict_schema_unchanged():
    mine = [(k, "x".join(str(d) for d in v.shape)) for k, v in build().state_dict().items()]
    ref = []
    with open(os.path.join(ROOT, "tests", "golden", "state_schema_sttflownet.txt")) as f:
        for line in f:
            n, _, shp = line.strip().partition(" ")
            ref.append((n, shp))
    assert mine == ref


def _py_row_map(B, D, H, W, ws, ss):
    """pad + roll + window_partition of the row indices (-1: padding token): what hip.window_slice_map builds on the device."""
    from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import window_partition
    Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
    idx = F.pad(torch.arange(B * D * H * W, dtype=torch.float64).view(B, D, H, W, 1), (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D), value=-1)
    if any(ss):
        idx = torch.roll(idx, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    m = window_partition(idx, ws).reshape(-1).long()
    return m.int(), m.numel() // (ws[0] * ws[1] * ws[2])


@pytest.mark.parametrize("shift", [(0, 0, 0), (1, 4, 4)])
def test_block_training_applies_drop_path_to_both_branches(monkeypatch, shift):
    """The training form of the block draws stochastic depth on the attention AND the MLP branch with its own rate (reference
    :313, :329); DropPath is the identity outside training.  The attention runs as its torch composition (SDF_ANN_ATTN_BWD=0) and
    the row map comes from the host, so the block's training path can be followed here without a GPU."""
    from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw
    blk = sw.SwinTransformerBlock3D(96, 3, (2, 9, 9), shift, drop_path=0.15).train()
    drop_path = sw.drop_path
    calls = []

    def rec(x, p, training):
        calls.append((tuple(x.shape), p, training))
        return x
    monkeypatch.setattr(sw, "drop_path", rec)
    monkeypatch.setattr(sw.SwinTransformerBlock3D, "_row_map", staticmethod(lambda B, D, H, W, ws, ss, dev: _py_row_map(B, D, H, W, ws, ss)))
    x = torch.randn(1, 2, 11, 20, 96, requires_grad=True)
    with hip.scoped_switches(SDF_ANN_ATTN_BWD="0"):
        y = blk(x)
    y.sum().backward()
    assert calls == [((1, 2, 11, 20, 96), 0.15, True)] * 2
    assert x.grad is not None and torch.isfinite(x.grad).all()
    # timm semantics: a sample is dropped (zero) or kept and scaled by 1 / keep; identity in eval
    z = torch.ones(64, 3, 5)
    torch.manual_seed(3)
    d = drop_path(z, 0.25, True)
    per = d.flatten(1)
    assert all(torch.all(r == 0) or torch.allclose(r, torch.full_like(r, 1 / 0.75)) for r in per)
    assert 0 < int((per[:, 0] == 0).sum()) < 64
    assert drop_path(z, 0.25, False) is z


def test_torch_attention_rows_equal_the_materialised_sequence():
    """The SDF_ANN_ATTN_BWD=0 composition over the row map equals pad + roll + partition -> attention -> reverse + roll + crop."""
    from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw
    torch.manual_seed(0)
    B, D, H, W, Cc, nH, ws, ss = 2, 2, 11, 20, 96, 3, (2, 9, 9), (1, 4, 4)
    attn = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True).double()
    qkv = torch.randn(B * D * H * W, 3 * Cc, dtype=torch.float64)
    pad = torch.randn(3 * Cc, dtype=torch.float64)
    bias = attn.position_bias()
    scale = torch.clamp(attn.logit_scale, max=4.605170185988092).exp().reshape(-1)
    Dp, Hp, Wp = 2, 18, 27
    mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, torch.device("cpu")).double()
    m, B_ = _py_row_map(B, D, H, W, ws, ss)
    got = sw.attention_rows_torch(qkv, m, B_, 162, pad, scale, bias, mask, nH)
    # the reference's order of operations, materialised
    x = F.pad(qkv.view(B, D, H, W, -1) - pad, (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D)) + pad
    x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    win = sw.window_partition(x, ws)
    q, k, v = win.view(B_, 162, 3, nH, 32).permute(2, 0, 3, 1, 4)
    a = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.view(1, nH, 1, 1) + bias
    a = (a.view(B_ // mask.shape[0], mask.shape[0], nH, 162, 162) + mask.view(1, -1, 1, 162, 162)).view(B_, nH, 162, 162)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(B_, 162, Cc)
    o = torch.roll(sw.window_reverse(o, ws, B, Dp, Hp, Wp), shifts=ss, dims=(1, 2, 3))[:, :D, :H, :W].reshape(-1, Cc)
    assert torch.allclose(got, o, rtol=0, atol=1e-12)
