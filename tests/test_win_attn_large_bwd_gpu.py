"""The window-attention backward above 192 tokens per window (csrc/win_attn_large_bwd.hip, through autograd.WinAttnAnnFunction /
WinAttnSewFunction, which pick `hip.win_attn_ann_bwd_large` / `hip.win_attn_sew_bwd_large` by N).

ANN against the fp64 materialised reference of tests/test_win_attn_ann_bwd_gpu.py (restated in win_attn_large_bwd_cases.py): dqkv,
d_pad (their q, k and v thirds each against its own largest element), d_logit_scale and every cpb_mlp gradient within 2e-5 of the
tensor's largest element.  SEW against fp64 autograd of the oracle's
`sew_attention_core`: dq, dk, dv, d_bias within 1e-5.  Those are the bounds of the <= 192 kernels' tests; measured on an MI355X the worst
case is 6.9e-6 (ANN, a cpb_mlp gradient at N = 450 shifted) and 2.1e-6 (SEW, dv at N = 450 masked), so no bound was widened.  For every case: two wrapper
calls and one call on buffers between guard regions are bit-equal, the guards and the inputs are unchanged, and the launch log of the
backward holds the kernels of the new file only."""
import ctypes as C
import zlib

import pytest
import torch

import win_attn_large_bwd_cases as LC
from routes_common import short
from sdformerflow_amd import hip
from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_ANN, TOL_SEW = 2e-5, 1e-5
ANN_KERNELS = ["win_attn_large_ann_bwd_query_kernel", "win_attn_large_ann_bwd_key_kernel", "win_attn_large_ann_bwd_dbias_kernel",
               "win_attn_large_bwd_sum_runs_kernel", "win_attn_large_ann_bwd_reduce_kernel"]
SEW_KERNELS = ["win_attn_large_sew_bwd_gram_kernel", "win_attn_large_sew_bwd_dv_kernel", "win_attn_large_sew_dbias_kernel", "win_attn_large_bwd_sum_runs_kernel"]
OLD_KERNELS = ("win_attn_ann_bwd_kernel", "win_attn_ann_bwd_reduce_kernel", "sew_bwd_kernel", "sew_bwd_dbias_kernel",
               "sew_bwd_dbias_finish_kernel")

# name: (ws, (B, D, H, W) or N = window-major rows with B_ = 2, shifted / masked, zero pad row, logit_scale of head 0 above ln 100)
# Row-mapped: one or two windows per axis, H and W no multiples of the window, so padding tokens exist (d_pad); N = 200 also pads D.
# Window-major: the first N tokens of the window (its position bias cut to N x N), so N need not be a window's volume.
ANN_CASES = {
    "n200": ((2, 10, 10), (1, 3, 11, 13), False, False, False),          # 13 tiles, 8 real tokens in the last
    "n200_shift": ((2, 10, 10), (1, 3, 11, 13), True, False, False),
    "n450": ((2, 15, 15), (1, 2, 16, 20), False, False, False),
    "n450_shift": ((2, 15, 15), (1, 2, 16, 20), True, False, True),      # ... and a clamped head
    "n450_zero_pad": ((2, 15, 15), (1, 2, 16, 20), False, True, False),
    "n968": ((2, 22, 22), (1, 2, 23, 30), False, False, False),
    "n968_shift": ((2, 22, 22), (1, 2, 23, 30), True, False, False),
    "wm193": ((2, 10, 10), 193, False, False, False),
    "wm256_mask": ((2, 8, 16), 256, True, False, False),
    "wm1024": ((2, 16, 32), 1024, False, False, False),
}
ANN_PARAMS = [(c, 96, 3) for c in ANN_CASES] + [("n450_shift", 384, 12)]


def _close(got, ref, tol, what):
    ref = ref.double()
    err, top = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"    {what}: max |got - ref| {err:.3e} = {err / max(top, 1e-300):.2e} of max |ref| {top:.3e}")
    assert err <= tol * top, (what, err, top)


def _close_thirds(got, ref, tol, what):
    """the q, k and v thirds of a (..., 3C) tensor, each against its own largest element"""
    Cc = ref.shape[-1] // 3
    for i, part in enumerate("qkv"):
        _close(got[..., i * Cc:(i + 1) * Cc], ref[..., i * Cc:(i + 1) * Cc], tol, f"{what}.{part}")


def _names(log):
    return [short(r[0]) for r in log.rows]


def _ann_guarded(qkv, row_map, B_, N, pad, scale, bias, mask, nH, dout):
    """sdf_win_attn_large_ann_bwd on buffers between guard regions -> (dqkv, d_pad, d_scale, d_bias); asserts guards and inputs"""
    rows, C3 = qkv.shape
    ins = {"qkv": qkv, "pad": pad, "scale": scale, "bias": bias, "dout": dout}
    if row_map is not None:
        ins["row_map"] = row_map
    if mask is not None:
        ins["mask"] = mask
    gi = {k: LC.guarded(tuple(v.shape), v.dtype, DEV, v) for k, v in ins.items()}
    nbytes = hip.lib().sdf_win_attn_large_ann_bwd_workspace_bytes(B_, nH, N)
    assert nbytes > 0 and nbytes % 256 == 0
    go = {"dqkv": LC.guarded((rows, C3), torch.float32, DEV), "d_pad": LC.guarded((C3,), torch.float32, DEV),
          "d_scale": LC.guarded((nH,), torch.float32, DEV), "d_bias": LC.guarded((nH, N, N), torch.float32, DEV),
          "ws": LC.guarded((nbytes // 4,), torch.float32, DEV)}
    p = lambda k: gi[k][1].data_ptr() if k in gi else None
    d = hip.WinAttnBwdDesc()
    d.qkv, d.row_map, d.pad_qkv, d.dout = p("qkv"), p("row_map"), p("pad"), p("dout")
    d.scale, d.bias, d.mask = p("scale"), p("bias"), p("mask")
    d.dqkv, d.d_pad, d.d_scale, d.d_bias = (go[k][1].data_ptr() for k in ("dqkv", "d_pad", "d_scale", "d_bias"))
    d.workspace, d.workspace_bytes = go["ws"][1].data_ptr(), nbytes
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, N, 32
    rc = hip.lib().sdf_win_attn_large_ann_bwd(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, (buf, mid) in gi.items():
        LC.guards_hold(buf, "input " + k)
        assert torch.equal(mid, ins[k]), f"input {k} was written"
    for k, (buf, mid) in go.items():
        LC.guards_hold(buf, "output " + k)
        if k != "ws":
            assert not torch.isnan(mid).any(), f"output {k}: an element was never written"
    return tuple(go[k][1] for k in ("dqkv", "d_pad", "d_scale", "d_bias"))


@pytest.mark.parametrize("case,Cc,nH", ANN_PARAMS)
def test_ann_backward_matches_fp64_materialised(case, Cc, nH):
    from sdformerflow_amd.autograd import WinAttnAnnFunction
    ws, grid, shifted, zero_pad, big = ANN_CASES[case]
    N = grid if isinstance(grid, int) else ws[0] * ws[1] * ws[2]
    g = torch.Generator().manual_seed(zlib.crc32(repr((Cc, case)).encode()))
    attn = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True)
    with torch.no_grad():
        for p in attn.cpb_mlp.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
        attn.logit_scale.copy_(torch.log(torch.full((nH, 1, 1), 10.0)) + 0.5 * torch.randn((nH, 1, 1), generator=g))
        if big:
            attn.logit_scale[0] = 5.0                          # above ln 100: clamped, no gradient
    attn = attn.to(DEV).train()
    if not isinstance(grid, int):
        B, D, H, W = grid
        ss = tuple(w // 2 for w in ws) if shifted else (0, 0, 0)
        Dp, Hp, Wp = D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]
        rows = B * D * H * W
        mask = sw.compute_mask(Dp, Hp, Wp, ws, ss, torch.device(DEV)).contiguous() if shifted else None
        row_map, B_ = hip.window_slice_map(B, D, H, W, ws, ss, DEV)
        assert int((row_map < 0).sum()) > 0                     # padding tokens exist
    else:
        B_, rows, row_map = 2, 2 * N, None
        mask = LC.label_mask(2, N, g).to(DEV).contiguous() if shifted else None
    qkv = torch.randn(rows, 3 * Cc, generator=g).to(DEV)
    pad = (torch.zeros(3 * Cc) if zero_pad else torch.randn(3 * Cc, generator=g)).to(DEV)
    dout = torch.randn(rows, Cc, generator=g).to(DEV)

    q32, p32 = qkv.clone().requires_grad_(True), pad.clone().requires_grad_(True)
    bias, scale = attn._bias_and_scale()
    bias = bias[:, :N, :N]
    o = WinAttnAnnFunction.apply(q32, scale, bias, p32, row_map, B_, N, mask, nH)
    with hip.launch_log() as log:
        (o * dout).sum().backward()
    names = _names(log)
    assert [n for n in names if "win_attn" in n or "sew_bwd" in n] == ANN_KERNELS, names
    assert not any(n in OLD_KERNELS for n in names), names

    ref_attn = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True).to(DEV)
    ref_attn.load_state_dict(attn.state_dict())
    ref_attn = ref_attn.double().train()
    q64, p64 = qkv.double().requires_grad_(True), pad.double().requires_grad_(True)
    if not isinstance(grid, int):
        LC.ann_reference(q64, p64, ref_attn, B, D, H, W, ws, ss, nH, dout.double())
    else:
        LC.ann_reference_windows(q64, ref_attn, B_, N, nH, None if mask is None else mask.double(), dout.double())

    print(f"ann large bwd {case} C {Cc}:")
    _close_thirds(q32.grad, q64.grad, TOL_ANN, "dqkv")
    if not isinstance(grid, int):
        _close_thirds(p32.grad, p64.grad, TOL_ANN, "d_pad")
    else:
        assert not p32.grad.any()                               # no padding token without a row map
    _close(attn.logit_scale.grad, ref_attn.logit_scale.grad, TOL_ANN, "d_logit_scale")
    if big:
        assert attn.logit_scale.grad[0].item() == 0.0
    for (n, a), b in zip(attn.cpb_mlp.named_parameters(), ref_attn.cpb_mlp.parameters()):
        _close(a.grad, b.grad, TOL_ANN, "cpb_mlp." + n)
    if zero_pad:                                                # k of a padding token is 0: the normalize eps carries its gradient
        assert p64.grad[Cc:2 * Cc].abs().max().item() > 1e6

    with torch.no_grad():
        args = (qkv, row_map, B_, N, pad, scale.detach().contiguous(), bias.detach().contiguous(), mask, nH, dout)
        r1, r2 = hip.win_attn_ann_bwd_large(*args), hip.win_attn_ann_bwd_large(*args)
        r3 = _ann_guarded(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(r1, r2, r3))


# name: (Tq, N1, B_, nW or 0 = no mask)
SEW_CASES = {
    "w450": (2, 225, 4, 0),
    "w450_mask": (2, 225, 4, 2),
    "w193": (1, 193, 3, 0),
    "w193_mask": (1, 193, 3, 3),
    "w256": (2, 128, 2, 0),
    "w256_mask": (2, 128, 2, 1),
    "w968": (2, 484, 2, 0),
    "w968_mask": (2, 484, 2, 2),
    "w1024": (1, 1024, 2, 0),
    "w1024_mask": (1, 1024, 2, 2),
}
SEW_PARAMS = [(c, 3) for c in SEW_CASES] + [("w450", 12), ("w450_mask", 12)]


def _sew_guarded(q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout):
    """sdf_win_attn_large_sew_bwd on buffers between guard regions -> (dq, dk, dv, d_bias); asserts guards and inputs"""
    N, Cc = Tq * N1, q.shape[-1]
    ins = {"q": q, "k": k, "v": v, "scale": scale, "bias": bias, "dout": dout}
    if mask is not None:
        ins["mask"] = mask
    gi = {n: LC.guarded(tuple(t.shape), t.dtype, DEV, t) for n, t in ins.items()}
    nbytes = hip.lib().sdf_win_attn_large_sew_bwd_workspace_bytes(B_, nH, N)
    assert nbytes > 0 and nbytes % 256 == 0
    go = {n: LC.guarded((Tq, B_, N1, Cc), torch.float32, DEV) for n in ("dq", "dk", "dv")}
    go["d_bias"] = LC.guarded((nH, N, N), torch.float32, DEV)
    go["ws"] = LC.guarded((nbytes // 4,), torch.float32, DEV)
    p = lambda n: gi[n][1].data_ptr() if n in gi else None
    d = hip.WinAttnSewBwdDesc()
    d.q, d.k, d.v, d.dout, d.scale, d.bias, d.mask = p("q"), p("k"), p("v"), p("dout"), p("scale"), p("bias"), p("mask")
    d.dq, d.dk, d.dv, d.d_bias = (go[n][1].data_ptr() for n in ("dq", "dk", "dv", "d_bias"))
    d.workspace, d.workspace_bytes = go["ws"][1].data_ptr(), nbytes
    d.B_, d.nW, d.nH, d.Tq, d.N1, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, Tq, N1, 32
    rc = hip.lib().sdf_win_attn_large_sew_bwd(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for n, (buf, mid) in gi.items():
        LC.guards_hold(buf, "input " + n)
        assert torch.equal(mid, ins[n]), f"input {n} was written"
    for n, (buf, mid) in go.items():
        LC.guards_hold(buf, "output " + n)
        if n != "ws":
            assert not torch.isnan(mid).any(), f"output {n}: an element was never written"
    return tuple(go[n][1] for n in ("dq", "dk", "dv", "d_bias"))


@pytest.mark.parametrize("case,nH", SEW_PARAMS)
def test_sew_backward_matches_fp64_autograd(case, nH):
    from sdformerflow_amd.autograd import WinAttnSewFunction
    Tq, N1, B_, nW = SEW_CASES[case]
    Cc, N, scale = 32 * nH, Tq * N1, 0.125
    g = torch.Generator().manual_seed(zlib.crc32(repr((case, nH)).encode()))
    q, k, v = ((torch.rand((Tq, B_, N1, Cc), generator=g) < p).float() for p in (0.3, 0.2, 0.25))
    bias = torch.randn((nH, N, N), generator=g)
    mask = LC.label_mask(nW, N, g) if nW else None
    dout = torch.randn((Tq, B_, N1, Cc), generator=g)
    z, rq, rk, rv, rb = LC.sew_reference(*(t.to(DEV) for t in (q, k, v)), scale, bias.to(DEV), None if mask is None else mask.to(DEV),
                                         Tq, N1, nH, dout.to(DEV))

    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    bd = bias.to(DEV).requires_grad_(True)
    md = None if mask is None else mask.to(DEV).contiguous()
    sc = torch.full((nH,), scale, device=DEV)
    out = WinAttnSewFunction.apply(qd, kd, vd, bd, sc, md, nH)
    print(f"sew large bwd {case} nH {nH}:")
    _close(out.detach(), z, TOL_SEW, "out")
    with hip.launch_log() as log:
        (out * dout.to(DEV)).sum().backward()
    names = _names(log)
    assert [n for n in names if "win_attn" in n or "sew_bwd" in n] == SEW_KERNELS, names
    assert not any(n in OLD_KERNELS for n in names), names
    for name, got, ref in (("dq", qd.grad, rq), ("dk", kd.grad, rk), ("dv", vd.grad, rv), ("d_bias", bd.grad, rb)):
        _close(got, ref.reshape(got.shape), TOL_SEW, name)

    u8 = [t.to(DEV).to(torch.uint8) for t in (q, k, v)]
    args = (*u8, sc, bias.to(DEV), md, nH, Tq, B_, N1, dout.to(DEV))
    r1, r2 = hip.win_attn_sew_bwd_large(*args), hip.win_attn_sew_bwd_large(*args)
    r3 = _sew_guarded(*args)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(r1, r2, r3))


def test_range_is_refused_without_a_launch():
    """N = 192 and N = 1025: SDF_E_SHAPE from both large wrappers before any launch; hip.win_attn_sew_bwd keeps refusing N = 194."""
    def refused(fn, *args):
        with hip.launch_log() as log, pytest.raises(hip.SdfError) as e:
            fn(*args)
        assert e.value.rc == hip.E_SHAPE and not log.rows, (e.value.rc, log.rows)
    for N in (192, 1025):
        qkv, dout = torch.zeros((2 * N, 288), device=DEV), torch.zeros((2 * N, 96), device=DEV)
        sc, bias = torch.ones(3, device=DEV), torch.zeros((3, N, N), device=DEV)
        refused(hip.win_attn_ann_bwd_large, qkv, None, 2, N, torch.zeros(288, device=DEV), sc, bias, None, 3, dout)
        Tq, N1 = (2, 96) if N == 192 else (1, 1025)
        s = torch.zeros((Tq, 2, N1, 96), dtype=torch.uint8, device=DEV)
        refused(hip.win_attn_sew_bwd_large, s, s, s, sc, bias, None, 3, Tq, 2, N1, torch.zeros((Tq, 2, N1, 96), device=DEV))
    big = torch.zeros((2, 1, 97, 96), dtype=torch.uint8, device=DEV)                                  # N = 194 > 192
    refused(hip.win_attn_sew_bwd, big, big, big, torch.ones(3, device=DEV), torch.zeros((3, 194, 194), device=DEV), None, 3, 2, 1, 97,
            torch.zeros((2, 1, 97, 96), device=DEV))
    qkv = torch.zeros((2 * 194, 288), device=DEV)
    refused(hip.win_attn_ann_bwd, qkv, None, 2, 194, torch.zeros(288, device=DEV), torch.ones(3, device=DEV),
            torch.zeros((3, 194, 194), device=DEV), None, 3, torch.zeros((2 * 194, 96), device=DEV))
    torch.cuda.synchronize()
