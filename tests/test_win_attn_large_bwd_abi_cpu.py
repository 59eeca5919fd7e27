"""CPU-side checks of sdf_win_attn_large_ann_bwd / sdf_win_attn_large_sew_bwd (csrc/win_attn_large_bwd.hip), the window-attention
backward for 192 < N <= 1024 tokens per window: the symbols are declared, bound and exported, every argument error of the <= 192 entry
points returns the same code in the same order - with dummy pointers, so everything is refused before any launch and no GPU is needed -
the workspace does not grow as B_ * nH * N^2, and the fp64 references of the GPU tests (win_attn_large_bwd_cases.py) equal autograd
through the project's torch compositions."""
import ctypes as C
import os
import re

import torch

import win_attn_large_bwd_cases as LC
from sdformerflow_amd import hip, train
from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
P = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_win_attn_large_ann_bwd_workspace_bytes", "sdf_win_attn_large_ann_bwd", "sdf_win_attn_large_sew_bwd_workspace_bytes",
       "sdf_win_attn_large_sew_bwd")


def loaded_lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def ann_desc(**kw):
    d = hip.WinAttnBwdDesc()
    d.qkv, d.dout, d.scale, d.bias, d.dqkv, d.d_scale, d.d_bias, d.workspace = (P,) * 8
    d.B_, d.nW, d.nH, d.N, d.hd = 4, 1, 3, kw.get("N", 450), 32
    d.workspace_bytes = 1 << 40
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def sew_desc(**kw):
    d = hip.WinAttnSewBwdDesc()
    d.q, d.k, d.v, d.dout, d.scale, d.bias, d.dq, d.dk, d.dv, d.d_bias, d.workspace = (P,) * 11
    d.B_, d.nW, d.nH, d.Tq, d.N1, d.hd = 4, 1, 3, 2, 225, 32
    d.workspace_bytes = 1 << 40
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def test_symbols_are_declared_bound_and_exported():
    lib = loaded_lib()
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES and hasattr(lib, name)
    for old, new in (("sdf_win_attn_ann_bwd", "sdf_win_attn_large_ann_bwd"), ("sdf_win_attn_sew_bwd", "sdf_win_attn_large_sew_bwd")):
        assert hip.SIGNATURES[new] == hip.SIGNATURES[old]
        assert hip.SIGNATURES[new + "_workspace_bytes"] == hip.SIGNATURES[old + "_workspace_bytes"]
    assert lib.sdf_win_attn_large_ann_bwd.restype is C.c_int and lib.sdf_win_attn_large_ann_bwd_workspace_bytes.restype is C.c_int64
    assert lib.sdf_version() == 107                             # additive exports keep the version
    assert hip.win_attn_ann_bwd_large and hip.win_attn_sew_bwd_large


def test_range_is_192_exclusive_to_1024_inclusive():
    lib = loaded_lib()
    ann = lambda **kw: lib.sdf_win_attn_large_ann_bwd(C.byref(ann_desc(**kw)), None)
    sew = lambda **kw: lib.sdf_win_attn_large_sew_bwd(C.byref(sew_desc(**kw)), None)
    for N in (192, 162, 1025, 0, -5):
        assert ann(N=N) == E_SHAPE, N
        assert lib.sdf_win_attn_large_ann_bwd_workspace_bytes(4, 3, N) == 0
        assert lib.sdf_win_attn_large_sew_bwd_workspace_bytes(4, 3, N) == 0
    assert sew(Tq=2, N1=96) == E_SHAPE and sew(Tq=1, N1=1025) == E_SHAPE and sew(Tq=2, N1=81) == E_SHAPE
    assert sew(Tq=0, N1=450) == E_SHAPE and sew(Tq=2, N1=0) == E_SHAPE
    for N in (193, 450, 1024):
        assert lib.sdf_win_attn_large_ann_bwd_workspace_bytes(4, 3, N) > 0 and lib.sdf_win_attn_large_sew_bwd_workspace_bytes(4, 3, N) > 0
    assert lib.sdf_win_attn_large_ann_bwd_workspace_bytes(0, 3, 450) == 0 and lib.sdf_win_attn_large_sew_bwd_workspace_bytes(4, 0, 450) == 0
    # the first two entry points are unchanged: 193 tokens and beyond are refused there
    assert lib.sdf_win_attn_ann_bwd(C.byref(ann_desc(N=193)), None) == E_SHAPE
    assert lib.sdf_win_attn_ann_bwd(C.byref(ann_desc(N=450)), None) == E_SHAPE
    assert lib.sdf_win_attn_sew_bwd(C.byref(sew_desc()), None) == E_SHAPE
    assert lib.sdf_win_attn_sew_bwd(C.byref(sew_desc(Tq=1, N1=194)), None) == E_SHAPE
    assert lib.sdf_win_attn_ann_bwd_workspace_bytes(4, 3, 450) == 0 and lib.sdf_win_attn_sew_bwd_workspace_bytes(4, 3, 450) == 0


def test_argument_errors_in_the_order_of_the_first_entry_points():
    """NULL pointers, then head_dim / the range, then B_ % nW, then the too-small workspace (all SDF_E_SHAPE), then the alignment - and
    the same descriptors at N = 162 get the same codes from sdf_win_attn_ann_bwd / sdf_win_attn_sew_bwd."""
    lib = loaded_lib()
    ann_ws, sew_ws = lib.sdf_win_attn_large_ann_bwd_workspace_bytes(4, 3, 450), lib.sdf_win_attn_large_sew_bwd_workspace_bytes(4, 3, 450)
    ann = lambda **kw: lib.sdf_win_attn_large_ann_bwd(C.byref(ann_desc(**kw)), None)
    sew = lambda **kw: lib.sdf_win_attn_large_sew_bwd(C.byref(sew_desc(**kw)), None)
    ann0 = lambda **kw: lib.sdf_win_attn_ann_bwd(C.byref(ann_desc(**dict({"N": 162}, **kw))), None)
    sew0 = lambda **kw: lib.sdf_win_attn_sew_bwd(C.byref(sew_desc(**dict({"N1": 81}, **kw))), None)
    assert lib.sdf_win_attn_large_ann_bwd(None, None) == E_NULL and lib.sdf_win_attn_large_sew_bwd(None, None) == E_NULL
    for f in ("qkv", "dout", "scale", "bias", "dqkv", "d_scale", "d_bias", "workspace"):
        assert ann(**{f: None}) == ann0(**{f: None}) == E_NULL, f
    assert ann(row_map=P) == ann0(row_map=P) == E_NULL                                  # the row map needs the pad row and d_pad
    assert ann(row_map=P, pad_qkv=P) == ann0(row_map=P, pad_qkv=P) == E_NULL
    for f in ("q", "k", "v", "dout", "scale", "bias", "dq", "dk", "dv", "d_bias", "workspace"):
        assert sew(**{f: None}) == sew0(**{f: None}) == E_NULL, f
    for one, first in ((ann, ann0), (sew, sew0)):
        assert one(hd=16) == first(hd=16) == E_SHAPE                                    # head dim must be 32
        assert one(B_=0) == first(B_=0) == E_SHAPE and one(nH=0) == first(nH=0) == E_SHAPE
        assert one(mask=P, nW=3) == first(mask=P, nW=3) == E_SHAPE                      # B_ % nW != 0
        assert one(mask=P, nW=0) == first(mask=P, nW=0) == E_SHAPE
        assert one(workspace_bytes=255) == first(workspace_bytes=255) == E_SHAPE        # too small
        assert one(workspace=P + 128) == first(workspace=P + 128) == E_ALIGN            # misaligned
        # order: NULL before the shape (head dim, range, windows per mask, workspace size) before the alignment
        assert one(bias=None, hd=16, workspace=P + 128) == first(bias=None, hd=16, workspace=P + 128) == E_NULL
        assert one(hd=16, workspace=P + 128) == first(hd=16, workspace=P + 128) == E_SHAPE
        assert one(mask=P, nW=3, workspace=P + 128) == first(mask=P, nW=3, workspace=P + 128) == E_SHAPE
        assert one(workspace_bytes=255, workspace=P + 128) == first(workspace_bytes=255, workspace=P + 128) == E_SHAPE
    assert ann(N=192, qkv=P + 8) == E_SHAPE and sew(Tq=1, N1=1025, dout=P + 4) == E_SHAPE
    assert ann(workspace_bytes=ann_ws - 1) == E_SHAPE and sew(workspace_bytes=sew_ws - 1) == E_SHAPE
    assert ann(workspace_bytes=ann_ws, qkv=P + 8) == E_ALIGN and sew(workspace_bytes=sew_ws, dout=P + 4) == E_ALIGN
    assert ann(qkv=P + 8) == ann0(qkv=P + 8) == E_ALIGN and ann(dout=P + 8) == ann0(dout=P + 8) == E_ALIGN
    assert ann(dqkv=P + 2) == ann0(dqkv=P + 2) == E_ALIGN
    assert ann(row_map=P, pad_qkv=P + 8, d_pad=P) == ann0(row_map=P, pad_qkv=P + 8, d_pad=P) == E_ALIGN
    assert sew(q=P + 2) == sew0(q=P + 2) == E_ALIGN and sew(dv=P + 8) == sew0(dv=P + 8) == E_ALIGN


def test_workspace_has_no_term_in_windows_times_tokens_squared():
    """ws(2 B_) - ws(B_) <= B_ nH (32 NP + 1024) bytes: per added window room for the row statistics and the d_pad / d_scale
    partials, none for an N^2 term (one window's fp32 score matrix at N = 450 is 810 000 bytes, the allowance 15 872 per head)."""
    lib = loaded_lib()
    nH = 3
    for fn in (lib.sdf_win_attn_large_ann_bwd_workspace_bytes, lib.sdf_win_attn_large_sew_bwd_workspace_bytes):
        for N in (450, 1024):
            NP = 16 * -(-N // 16)
            for B_ in (256, 512, 1024):
                a, b = fn(B_, nH, N), fn(2 * B_, nH, N)
                assert 0 < a <= b and b - a <= B_ * nH * (32 * NP + 1024), (N, B_, a, b)


def test_wrappers_and_autograd_pick_the_entry_point_by_window_size(monkeypatch):
    """hip.win_attn_*_bwd stay on the first entry points, hip.win_attn_*_bwd_large call the new ones, and the autograd Functions'
    backward picks by N as hip._win_attn_fwd picks the forward."""
    from sdformerflow_amd import autograd
    calls = []
    for name in ("win_attn_ann_bwd", "win_attn_ann_bwd_large", "win_attn_sew_bwd", "win_attn_sew_bwd_large"):
        monkeypatch.setattr(hip, name, lambda *a, _n=name: (calls.append(_n), (None,) * 4)[1])

    class Ctx:
        pass
    for N, want in ((162, "win_attn_ann_bwd"), (192, "win_attn_ann_bwd"), (193, "win_attn_ann_bwd_large"), (1024, "win_attn_ann_bwd_large")):
        ctx = Ctx()
        ctx.saved_tensors, ctx.cfg = (None,) * 4, (None, 2, N, None, 3)
        autograd.WinAttnAnnFunction.backward(ctx, torch.zeros(1))
        assert calls[-1] == want, (N, calls)
    for (Tq, N1), want in (((2, 96), "win_attn_sew_bwd"), ((1, 193), "win_attn_sew_bwd_large"), ((2, 225), "win_attn_sew_bwd_large")):
        ctx = Ctx()
        ctx.saved_tensors, ctx.cfg = (torch.zeros((Tq, 1, N1, 96), dtype=torch.uint8),) * 3 + (None,), (None, None, 3, torch.float32)
        try:
            autograd.WinAttnSewFunction.backward(ctx, torch.zeros(1))
        except AttributeError:                                  # (the stub's None results have no .to(): the call was made)
            pass
        assert calls[-1] == want, ((Tq, N1), calls)


def test_switch_value_2_opts_in_up_to_1024_tokens():
    import pytest
    for switch in ("SDF_ANN_ATTN_BWD", "SDF_SEW_ATTN_BWD"):
        for value in (None, "1"):
            with hip.scoped_switches(**{switch: value}):
                hip.check_attn_bwd_window(192, switch)
                with pytest.raises(NotImplementedError, match=f"{switch}=0") as e:
                    hip.check_attn_bwd_window(450, switch)
                assert "192" in str(e.value) and f"{switch}=2" in str(e.value)
        with hip.scoped_switches(**{switch: "0"}):
            hip.check_attn_bwd_window(450, switch)
            hip.check_attn_bwd_window(4000, switch)
        with hip.scoped_switches(**{switch: "2"}):
            for N in (162, 192, 193, 450, 1024):
                hip.check_attn_bwd_window(N, switch)
            with pytest.raises(NotImplementedError, match="1024"):
                hip.check_attn_bwd_window(1025, switch)


def test_fp64_references_equal_autograd_through_the_torch_compositions():
    """N = 200, ws (2,10,10) on a 3 x 11 x 13 grid (padding along every axis), shifted: the materialised ANN reference against
    `attention_rows_torch` over the host row map, and the SEW reference against `train.sew_attention_core_torch`, in fp64 to 1e-10."""
    g = torch.Generator().manual_seed(11)
    B, D, H, W, Cc, nH, ws, ss = 1, 3, 11, 13, 96, 3, (2, 10, 10), (1, 5, 5)
    N = 200
    a1 = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True).double().train()
    a2 = sw.WindowAttention3D(Cc, ws, (0, 0, 0), nH, qkv_bias=True).double().train()
    a2.load_state_dict(a1.state_dict())
    qkv = torch.randn(B * D * H * W, 3 * Cc, generator=g, dtype=torch.float64)
    pad = torch.randn(3 * Cc, generator=g, dtype=torch.float64)
    dout = torch.randn(B * D * H * W, Cc, generator=g, dtype=torch.float64)
    q1, p1 = qkv.clone().requires_grad_(True), pad.clone().requires_grad_(True)
    LC.ann_reference(q1, p1, a1, B, D, H, W, ws, ss, nH, dout)
    q2, p2 = qkv.clone().requires_grad_(True), pad.clone().requires_grad_(True)
    m, B_ = LC.py_row_map(B, D, H, W, ws, ss)
    assert B_ == 8 and int((m < 0).sum()) > 0
    mask = sw.compute_mask(4, 20, 20, ws, ss, torch.device("cpu")).double()
    bias, scale = a2._bias_and_scale()
    (sw.attention_rows_torch(q2, m, B_, N, p2, scale, bias, mask, nH) * dout).sum().backward()
    pairs = [("dqkv", q1.grad, q2.grad), ("d_pad", p1.grad, p2.grad), ("d_logit_scale", a1.logit_scale.grad, a2.logit_scale.grad)]
    pairs += [("cpb_mlp." + n, x.grad, y.grad) for (n, x), y in zip(a1.cpb_mlp.named_parameters(), a2.cpb_mlp.parameters())]
    for what, x, y in pairs:
        assert (x - y).abs().max().item() <= 1e-10 * max(y.abs().max().item(), 1.0), what

    Tq, N1, B_ = 2, 100, 4
    q, k, v = ((torch.rand((Tq, B_, N1, Cc), generator=g) < p).double() for p in (0.3, 0.2, 0.25))
    # The composition computes in fp32 by design.  Bias in eighths, dO in small integers, scale 1/8, mask 0 / -100: every intermediate
    # is a multiple of 1/64 below 2^24 of them, so its fp32 arithmetic is exact and the two sides can be compared to 1e-10.
    sbias = torch.randint(-16, 17, (nH, N, N), generator=g).double() / 8
    smask = LC.label_mask(2, N, g).double()
    sdout = torch.randint(-3, 4, (Tq, B_, N1, Cc), generator=g).double()
    z, rq, rk, rv, rb = LC.sew_reference(q, k, v, 0.125, sbias, smask, Tq, N1, nH, sdout)
    t = [x.float().requires_grad_(True) for x in (q, k, v, sbias)]
    z32 = train.sew_attention_core_torch(t[0], t[1], t[2], torch.full((nH,), 0.125), t[3], smask.float(), nH)
    (z32 * sdout.float()).sum().backward()
    assert (z32.double() - z).abs().max().item() <= 1e-10 * z.abs().max().item()
    for what, x, y in (("dq", rq, t[0].grad), ("dk", rk, t[1].grad), ("dv", rv, t[2].grad), ("d_bias", rb, t[3].grad)):
        assert (x - y.double()).abs().max().item() <= 1e-10 * max(y.abs().max().item(), 1.0), what
