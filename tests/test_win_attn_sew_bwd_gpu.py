"""Backward of the SEW spiking window attention (csrc/win_attn_sew_bwd.hip through autograd.WinAttnSewFunction) against fp64 autograd
of the oracle's `sew_attention_core` (reference Spiking_swin_transformer3D.py:320-363): dq, dk, dv and d_bias each within 1e-5 of the
tensor's largest element; the forward `out` per element within 1e-5 (|attn| @ v), the bound of test_win_attn_fwd_gpu.py (one relative
to the largest element would let 0.04 through under a -100 mask); two calls bit-equal; shapes outside the kernel's set refused with
SDF_E_SHAPE.  Per element and per kernel route: test_win_attn_bwd_routes_gpu.py."""
import zlib

import pytest
import torch

from oracle import sdformer_oracle as O
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
CASES = {                   # name: (Tq, N1, B_, nW or 0 = no mask)
    "w162": (2, 81, 12, 0),
    "w162_mask": (2, 81, 12, 6),
    "w128": (2, 64, 8, 0),
    "w128_mask": (2, 64, 8, 4),
    "trunc_tq1": (1, 45, 6, 0),          # a truncated window of a small stage map: depth 1, 5 x 9 tokens
    "trunc_tq1_mask": (1, 45, 6, 3),
    "edge192": (2, 96, 4, 2),            # the largest window the kernel takes (N = 192)
    "edge1": (1, 1, 3, 0),               # a one-token window
}


def _inputs(case, nH):
    Tq, N1, B_, nW = CASES[case]
    Cc, N = 32 * nH, Tq * N1
    g = torch.Generator().manual_seed(zlib.crc32(repr((case, nH)).encode()))
    q, k, v = ((torch.rand((Tq, B_, N1, Cc), generator=g) < p).float() for p in (0.3, 0.2, 0.25))
    bias = torch.randn((nH, N, N), generator=g)
    mask = None
    if nW:
        lab = torch.randint(0, 3, (nW, N), generator=g)
        mask = torch.where(lab[:, :, None] != lab[:, None, :], torch.tensor(-100.0), torch.tensor(0.0))
    dout = torch.randn((Tq, B_, N1, Cc), generator=g)
    return q, k, v, bias, mask, dout


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("nH", [3, 12])
@pytest.mark.parametrize("scale", [0.125, 1.0])
def test_sew_attention_backward_matches_fp64_autograd(case, nH, scale):
    from sdformerflow_amd.autograd import WinAttnSewFunction
    Tq, N1, B_, _ = CASES[case]
    q, k, v, bias, mask, dout = _inputs(case, nH)
    r = [t.double().reshape(B_, nH, Tq * N1, 32).requires_grad_(True) for t in (q, k, v)]
    rb = bias.double().requires_grad_(True)
    z, attn = O.sew_attention_core(r[0], r[1], r[2], scale, rb, None if mask is None else mask.double(), Tq, N1)
    bound = TOL * (attn.detach().abs() @ r[2].detach()).reshape(B_, nH, Tq, N1, 32).permute(2, 0, 3, 1, 4).reshape(z.shape)   # z's scramble
    (z * dout.double()).sum().backward()

    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    bd = bias.to(DEV).requires_grad_(True)
    md = None if mask is None else mask.to(DEV).contiguous()
    sc = torch.full((nH,), scale, device=DEV)
    out = WinAttnSewFunction.apply(qd, kd, vd, bd, sc, md, nH)
    assert bool(((out.cpu().double() - z.detach()).abs() <= bound).all()), ((out.cpu().double() - z.detach()).abs() / bound).max().item() * TOL
    (out * dout.to(DEV)).sum().backward()
    for name, got, ref in (("dq", qd.grad, r[0].grad), ("dk", kd.grad, r[1].grad), ("dv", vd.grad, r[2].grad), ("d_bias", bd.grad, rb.grad)):
        ref = ref.reshape(got.shape)
        err = (got.cpu().double() - ref).abs().max().item()
        assert err <= TOL * ref.abs().max().item(), (name, err, ref.abs().max().item())

    u8 = [t.to(DEV).to(torch.uint8) for t in (q, k, v)]
    args = (*u8, sc, bias.to(DEV), md, nH, Tq, B_, N1, dout.to(DEV))
    r1, r2 = hip.win_attn_sew_bwd(*args), hip.win_attn_sew_bwd(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))


def test_sew_attention_backward_refuses_unsupported_shapes():
    def expect_shape(*args):
        with pytest.raises(hip.SdfError) as e:
            hip.win_attn_sew_bwd(*args)
        assert e.value.rc == hip.E_SHAPE
    q = torch.zeros((2, 4, 81, 96), dtype=torch.uint8, device=DEV)
    dout = torch.zeros((2, 4, 81, 96), device=DEV)
    sc, bias = torch.ones(3, device=DEV), torch.zeros((3, 162, 162), device=DEV)
    expect_shape(q, q, q, torch.ones(6, device=DEV), torch.zeros((6, 162, 162), device=DEV), None, 6, 2, 4, 81, dout)   # head_dim 16
    big = torch.zeros((2, 1, 97, 96), dtype=torch.uint8, device=DEV)                                                    # N = 194 > 192
    expect_shape(big, big, big, sc, torch.zeros((3, 194, 194), device=DEV), None, 3, 2, 1, 97, torch.zeros((2, 1, 97, 96), device=DEV))
    expect_shape(q, q, q, sc, bias, torch.zeros((3, 162, 162), device=DEV), 3, 2, 4, 81, dout)                          # 4 windows, 3 masks
    torch.cuda.synchronize()
