"""Shared by test_win_attn_large_bwd_gpu.py and test_win_attn_large_bwd_abi_cpu.py (csrc/win_attn_large_bwd.hip): the fp64 references
of the two attention backward passes, the host row map, and buffers between guard regions.

ANN: `ann_reference` restates `_reference` of tests/test_win_attn_ann_bwd_gpu.py - the reference's pad, roll and window partition
materialised (swin_transformer3D_v2.py:286-310, :176-202) - and `ann_reference_windows` is the same attention on rows that are
window-major already (no row map).  SEW: `sew_reference` is autograd through the oracle's `sew_attention_core`."""
import math

import torch
import torch.nn.functional as F

from oracle import sdformer_oracle as O
from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw

GUARD = 4096                  # elements on either side of a guarded buffer (a multiple of 256 bytes for every dtype used)


def py_row_map(B, D, H, W, ws, ss):
    """pad + roll + window_partition of the row indices (-1: padding token): what hip.window_slice_map builds on the device."""
    Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
    idx = F.pad(torch.arange(B * D * H * W, dtype=torch.float64).view(B, D, H, W, 1), (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D), value=-1)
    if any(ss):
        idx = torch.roll(idx, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    m = sw.window_partition(idx, ws).reshape(-1).long()
    return m.int(), m.numel() // (ws[0] * ws[1] * ws[2])


def _ann_windows(win, attn, nH, mask):
    """(B_, N, 3C) windows -> (B_, N, C), the module's parameters under autograd (N below the window's volume: its first N tokens)"""
    B_, N = win.shape[:2]
    q, k, v = win.view(B_, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
    scale = torch.clamp(attn.logit_scale, max=math.log(100.0)).exp()
    a = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1) * scale.view(1, nH, 1, 1) + attn.position_bias()[:, :N, :N]
    if mask is not None:
        nW = mask.shape[0]
        a = (a.view(B_ // nW, nW, nH, N, N) + mask.view(1, nW, 1, N, N)).view(B_, nH, N, N)
    return (a.softmax(-1) @ v).transpose(1, 2).reshape(B_, N, -1)


def ann_reference(qkv, pad, attn, B, D, H, W, ws, ss, nH, dout):
    """fp64, materialised: pad (padding rows read `pad`) -> roll -> partition -> attention -> reverse -> roll back -> crop; leaves the
    gradients in qkv.grad, pad.grad and the module's parameters.  The pad row is selected into the padding positions: pad.grad is the sum
    over those positions alone, its q third exactly 0 (a padding token's dO, so its row of dS, is 0)."""
    Cc = qkv.shape[1] // 3
    Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
    grow = (0, 0, 0, Wp - W, 0, Hp - H, 0, Dp - D)
    real = F.pad(torch.ones((B, D, H, W, 1), dtype=qkv.dtype, device=qkv.device), grow) > 0
    x = torch.where(real, F.pad(qkv.view(B, D, H, W, -1), grow), pad)      # (not pad(qkv - pad) + pad: d_pad would be a cancelling difference)
    shifted = any(ss)
    if shifted:
        x = torch.roll(x, shifts=tuple(-s for s in ss), dims=(1, 2, 3))
    mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, qkv.device).double() if shifted else None
    o = _ann_windows(sw.window_partition(x, ws), attn, nH, mask)
    o = sw.window_reverse(o, ws, B, Dp, Hp, Wp)
    if shifted:
        o = torch.roll(o, shifts=ss, dims=(1, 2, 3))
    (o[:, :D, :H, :W].reshape(-1, Cc) * dout).sum().backward()


def ann_reference_windows(qkv, attn, B_, N, nH, mask, dout):
    """fp64, rows window-major (B_ * N, 3C): the same attention without a row map."""
    (_ann_windows(qkv.view(B_, N, -1), attn, nH, mask).reshape(B_ * N, -1) * dout).sum().backward()


def sew_reference(q, k, v, scale, bias, mask, Tq, N1, nH, dout):
    """fp64 autograd of the oracle's core: q, k, v (T', B_, N1, C) spikes as floats -> (z, dq, dk, dv (T', B_, N1, C), d_bias)"""
    B_ = q.shape[1]
    r = [t.detach().double().reshape(B_, nH, Tq * N1, 32).clone().requires_grad_(True) for t in (q, k, v)]
    rb = bias.detach().double().clone().requires_grad_(True)
    z, _ = O.sew_attention_core(r[0], r[1], r[2], scale, rb, None if mask is None else mask.double(), Tq, N1)
    (z * dout.double()).sum().backward()
    return (z.detach(), *(t.grad.reshape(q.shape) for t in r), rb.grad)


def label_mask(nW, N, g):
    """(nW, N, N) of 0 / -100: tokens of three random groups per window do not see each other (the shape of a shift mask)"""
    lab = torch.randint(0, 3, (nW, N), generator=g)
    return torch.where(lab[:, :, None] != lab[:, None, :], torch.tensor(-100.0), torch.tensor(0.0))


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
_FILL = {torch.float32: float("nan"), torch.uint8: 7, torch.int32: -7}


def guarded(shape, dtype, device, fill=None):
    """(buffer with GUARD elements of a marker (NaN / 7 / -7) on either side, its middle viewed as `shape`): `fill` copied in, or the
    marker left where an output belongs"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), _FILL[dtype], dtype=dtype, device=device)
    mid = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        mid.copy_(fill)
    assert mid.data_ptr() % 256 == 0
    return buf, mid


def guards_hold(buf, what):
    """both guard regions still hold the marker, bit for bit"""
    n = buf.numel() - 2 * GUARD
    bits = buf.view(torch.int32) if buf.dtype == torch.float32 else buf
    mark = torch.full((1,), _FILL[buf.dtype], dtype=buf.dtype).view(bits.dtype).item()
    assert bool((bits[:GUARD] == mark).all()) and bool((bits[GUARD + n:] == mark).all()), f"{what}: a guard element was written"
