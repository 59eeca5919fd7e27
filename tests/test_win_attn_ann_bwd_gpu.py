"""Backward of the ANN cosine window attention (csrc/win_attn_bwd.hip through autograd.WinAttnAnnFunction) against an fp64 torch
composition that materialises the reference's pad, roll and window partition (swin_transformer3D_v2.py:286-310, :176-202):
dqkv, d_pad (the padding tokens' share of the qkv bias gradient), d_logit_scale (through the clamp) and the cpb_mlp gradients,
each within 2e-5 of the tensor's largest element (the forward's bound) - the q, k and v thirds of dqkv and of d_pad each against
their own largest element (with a zero pad row the k third of d_pad exceeds 1e6 and would hide the other two); two backward calls
bit-equal.  Per element and per kernel route: test_win_attn_bwd_routes_gpu.py."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from sdformerflow_amd import hip
from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw

pytestmark = pytest.mark.gpu

TOL = 2e-5
CASES = {                    # name: (B, D, H, W, shifted, zero pad row, logit_scale of head 0 above ln 100)
    "plain": (2, 2, 18, 18, False, False, False),
    "shift_pad": (1, 2, 11, 20, True, False, False),
    "zero_pad": (1, 2, 11, 20, False, True, False),
    "big_scale": (2, 2, 11, 20, True, False, True),
}


def _reference(qkv, pad, attn, B, D, H, W, ws, ss, nH, dout):
    """fp64, materialised: pad (padding rows read `pad`) -> roll -> partition -> attention -> reverse -> roll back -> crop.  The pad row
    is selected into the padding positions, so its gradient is the sum over those positions alone and its q third is exactly 0 (a
    padding token's output is cropped: its dO, so its row of dS, is 0), as the kernel's is."""
    Cc = qkv.shape[1] // 3
    Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
    grow = (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D)
    real = F.pad(torch.ones((B, D, H, W, 1), dtype=qkv.dtype, device=qkv.device), grow) > 0
    x = torch.where(real, F.pad(qkv.view(B, D, H, W, -1), grow), pad)      # (not pad(qkv - pad) + pad: d_pad would be a cancelling difference)
    shifted = any(ss)
    if shifted:
        x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    win = sw.window_partition(x, ws)
    B_, N = win.shape[:2]
    q, k, v = win.view(B_, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
    scale = torch.clamp(attn.logit_scale, max=math.log(100.0)).exp()
    a = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.view(1, nH, 1, 1) + attn.position_bias()
    if shifted:
        mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, qkv.device).double()
        nW = mask.shape[0]
        a = (a.view(B_ // nW, nW, nH, N, N) + mask.view(1, nW, 1, N, N)).view(B_, nH, N, N)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, Cc)
    o = sw.window_reverse(o, ws, B, Dp, Hp, Wp)
    if shifted:
        o = torch.roll(o, shifts=ss, dims=(1, 2, 3))
    (o[:, :D, :H, :W].reshape(-1, Cc) * dout).sum().backward()


def _close(got, ref, what):
    ref = ref.double()
    err = (got.double() - ref).abs().max().item()
    assert err <= TOL * ref.abs().max().item(), (what, err, ref.abs().max().item())


def _close_thirds(got, ref, what):
    """the q, k and v thirds of a (..., 3C) tensor, each against its own largest element"""
    Cc = ref.shape[-1] // 3
    for i, part in enumerate("qkv"):
        _close(got[..., i * Cc:(i + 1) * Cc], ref[..., i * Cc:(i + 1) * Cc], f"{what}.{part}")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("ws", [(2, 9, 9), (2, 7, 7)])
@pytest.mark.parametrize("Cc,nH", [(96, 3), (192, 6), (384, 12)])
def test_attention_backward_matches_fp64_materialised(Cc, nH, ws, case):
    B, D, H, W, shifted, zero_pad, big = CASES[case]
    ss = tuple(w // 2 for w in ws) if shifted else (0, 0, 0)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(zlib.crc32(repr((Cc, ws, case)).encode()))
    attn = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True)
    with torch.no_grad():
        for p in attn.cpb_mlp.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        attn.logit_scale.copy_(torch.log(torch.full((nH, 1, 1), 10.0)) + 0.5 * torch.randn((nH, 1, 1), generator=g))
        if big:
            attn.logit_scale[0] = 5.0                          # above ln 100: clamped, no gradient
    attn = attn.to(dev).train()
    rows = B * D * H * W
    qkv = torch.randn(rows, 3 * Cc, generator=g).to(dev)
    pad = torch.zeros(3 * Cc) if zero_pad else torch.randn(3 * Cc, generator=g)
    pad = pad.to(dev)
    dout = torch.randn(rows, Cc, generator=g).to(dev)

    Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
    mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, dev).contiguous() if shifted else None
    row_map, B_ = hip.window_slice_map(B, D, H, W, ws, ss, dev)
    N = ws[0] * ws[1] * ws[2]
    q32, p32 = qkv.clone().requires_grad_(True), pad.clone().requires_grad_(True)
    from sdformerflow_amd.autograd import WinAttnAnnFunction
    bias, scale = attn._bias_and_scale()
    o = WinAttnAnnFunction.apply(q32, scale, bias, p32, row_map, B_, N, mask, nH)
    (o * dout).sum().backward()

    ref_attn = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True).to(dev)
    ref_attn.load_state_dict(attn.state_dict())
    ref_attn = ref_attn.double().train()
    q64, p64 = qkv.double().requires_grad_(True), pad.double().requires_grad_(True)
    _reference(q64, p64, ref_attn, B, D, H, W, ws, ss, nH, dout.double())

    _close_thirds(q32.grad, q64.grad, "dqkv")
    _close_thirds(p32.grad, p64.grad, "d_pad")
    _close(attn.logit_scale.grad, ref_attn.logit_scale.grad, "d_logit_scale")
    if big:
        assert attn.logit_scale.grad[0].item() == 0.0
    for (n, a), b in zip(attn.cpb_mlp.named_parameters(), ref_attn.cpb_mlp.parameters()):
        _close(a.grad, b.grad, "cpb_mlp." + n)
    if zero_pad:                                                # k of a padding token is 0: the normalize eps carries its gradient
        assert p64.grad[Cc:2 * Cc].abs().max().item() > 1e6

    # deterministic: two calls of the kernel give bit-equal results
    with torch.no_grad():
        args = (qkv, row_map, B_, N, pad, scale.detach(), bias.detach(), mask, nH, dout)
        r1, r2 = hip.win_attn_ann_bwd(*args), hip.win_attn_ann_bwd(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
