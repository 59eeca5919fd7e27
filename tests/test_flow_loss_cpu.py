"""Host side of the HIP train-step head (csrc/flow_loss.hip), no GPU: an fp64 restatement of the kernel's formulas against the stored
results of the reference's loss class (tests/golden/flow_loss.npz, made by tests/golden/make_golden_flow_loss.py) and against
train.flow_loss_supervised in fp64; F.interpolate's nearest index map at the factors the kernel serves; every refusal of the C entry
with dummy pointers; the header, the signature table and the build list; the Python-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (1, 2, 4, 8, 16)
NEW = ("sdf_flow_loss_workspace_bytes", "sdf_flow_loss_fwd")


def restate64(preds, label, mask, n, flow_scaling=1.0, lambda_mod=1.0):
    """csrc/flow_loss.hip's formulas in fp64 on the CPU.  preds: list of (T, B, 2, h, w) tensors of any float dtype (a 16-bit f is rounded
    once to that dtype when T > 1, as the kernel and torch's reduction do); label (B, 2, H, W); mask (B, H, W) or (B, 1, H, W); n the
    valid-pixel count.  Returns a dict: `loss`, `grads` [(B, 2, h, w)] = d loss / d preds[i].sum(0), `records` (levels, B), and the same
    three expressions with every term replaced by its absolute value (|f fs| + |label| in place of the difference): `A_loss`,
    `A_grads`, `A_records` - the magnitudes the fp32 rounding errors scale with."""
    label = torch.as_tensor(label).detach().cpu().double()
    B, _, H, W = label.shape
    mask = torch.as_tensor(mask).detach().cpu().double().reshape(B, 1, H, W)
    L, np_ = len(preds), float(n) + 1e-9
    k = flow_scaling * lambda_mod / (L * B * np_)
    grads, records, a_grads, a_records = [], [], [], []
    for p in preds:
        p = torch.as_tensor(p).detach().cpu()
        f = p.double().sum(0)
        if p.dtype in (torch.bfloat16, torch.float16) and p.shape[0] > 1:
            f = f.to(p.dtype).double()
        h, w = f.shape[-2:]
        s = H // h
        assert (h * s, w * s) == (H, W)
        flow = f.repeat_interleave(s, -2).repeat_interleave(s, -1) * flow_scaling
        d = flow - label
        r = torch.sqrt((d * d).sum(1, keepdim=True) + 1e-8)
        records.append((r * mask).sum((1, 2, 3)))
        grads.append((mask * d / r * k).reshape(B, 2, h, s, w, s).sum((3, 5)))
        D = flow.abs() + label.abs()
        R = torch.sqrt((D * D).sum(1, keepdim=True) + 1e-8)
        a_records.append((R * mask.abs()).sum((1, 2, 3)))
        a_grads.append((mask.abs() * D / R * abs(k)).reshape(B, 2, h, s, w, s).sum((3, 5)))
    records, a_records = torch.stack(records), torch.stack(a_records)
    form = lambda rec, lam: float((lam * rec / np_).sum(0).mean() / L)
    return {"loss": form(records, lambda_mod), "grads": grads, "records": records, "A_loss": form(a_records, abs(lambda_mod)),
            "A_grads": a_grads, "A_records": a_records}


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "flow_loss.npz"))
    preds = [torch.from_numpy(z[f"pred{i}"]) for i in range(3)]
    return z, preds, torch.from_numpy(z["label"]), torch.from_numpy(z["mask"]), float(z["flow_scaling"]), float(z["lambda_mod"])


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max())


def test_restatement_reproduces_the_reference_class_in_fp64():
    """The fixture's fp64 loss and gradients (the reference class behind sum(0) and F.interpolate, autograd down to the raw
    predictions) to 1e-12 relative; every time step carries the same gradient, and fp32 autograd sits at fp32 distance."""
    z, preds, label, mask, fs, lam = golden()
    assert [label.shape[-1] // p.shape[-1] for p in preds] == [4, 2, 1] and preds[0].shape[:2] == (3, 2)
    assert bool((preds[-1].sum(0) * fs == label)[:, :, 3, 5:9].all())                   # the exact hits are in the fixture
    r = restate64(preds, label, mask, float(mask.sum()), fs, lam)
    assert abs(r["loss"] - float(z["loss64"])) <= 1e-12 * abs(float(z["loss64"]))
    for i, g in enumerate(r["grads"]):
        ref = torch.from_numpy(z[f"grad64_{i}"])
        assert ref.shape == preds[i].shape
        for t in range(ref.shape[0]):
            assert rel(g, ref[t]) <= 1e-12, (i, t)
        assert rel(torch.from_numpy(z[f"grad32_{i}"])[0], g) < 1e-5
        assert bool((g[:, :, 3, 5:9] == 0).all()) if i == 2 else True                   # d == 0 exactly: the gradient is an exact zero
    assert abs(float(z["loss32"]) - r["loss"]) < 1e-6 * r["loss"]
    assert r["A_loss"] >= r["loss"] and bool((r["A_records"] >= r["records"]).all())


@pytest.mark.parametrize("given_n", [False, True])
def test_restatement_agrees_with_the_package_loss_in_fp64(given_n):
    from sdformerflow_amd import train
    _, preds, label, mask, fs, lam = golden()
    n = torch.tensor(1234.0, dtype=torch.float64) if given_n else None
    leaves = [p.double().requires_grad_(True) for p in preds]
    flows = train._flows_of_preds(leaves, *label.shape[-2:])
    loss = train.flow_loss_supervised(flows, label.double(), mask.double(), fs, lam, n_valid=n)
    loss.backward()
    r = restate64(preds, label, mask, 1234.0 if given_n else float(mask.sum()), fs, lam)
    assert abs(r["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    for g, leaf in zip(r["grads"], leaves):
        assert rel(g, leaf.grad[0]) <= 1e-12 and torch.equal(leaf.grad[0], leaf.grad[-1])


@pytest.mark.parametrize("s", FACTORS)
def test_nearest_upsampling_reads_dst_floordiv_s(s):
    """F.interpolate(scale_factor=(H / h, W / w)), as the models call it, reads source index dst // s along both axes for every source
    size up to 16 * 40 / s: its fp32 floor(dst * (1 / s)) is exact at these factors, which is why the kernel may index with a shift."""
    for n in range(1, 16 * 40 // s + 1):
        src = torch.arange(n, dtype=torch.float32)
        want = torch.arange(n * s) // s
        rows = F.interpolate(src.view(1, 1, n, 1).expand(1, 1, n, 2), scale_factor=(n * s / n, 2 * s / 2))
        cols = F.interpolate(src.view(1, 1, 1, n).expand(1, 1, 2, n), scale_factor=(2 * s / 2, n * s / n))
        assert rows.shape == (1, 1, n * s, 2 * s) and cols.shape == (1, 1, 2 * s, n * s)
        assert torch.equal(rows[0, 0, :, 0].long(), want) and torch.equal(cols[0, 0, 0, :].long(), want), n


def test_new_entry_points_are_declared_and_bound():
    import test_abi_cpu
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    assert "typedef struct SdfFlowLossDesc" in hdr
    assert hip.SIGNATURES["sdf_flow_loss_fwd"] == (C.c_int, (C.POINTER(hip.FlowLossDesc), C.c_void_p))
    assert hip.SIGNATURES["sdf_flow_loss_workspace_bytes"] == (C.c_int64, (C.c_int,) * 4)
    names = list(hip.SIGNATURES)
    assert names.index("sdf_flow_loss_workspace_bytes") == names.index("sdf_flow_metrics_fwd") + 1      # beside the metrics
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107                        # (additive exports)
    assert hip.FLOW_LOSS_MAX_LEVELS == int(re.search(r"#define\s+SDF_FLOW_LOSS_MAX_LEVELS\s+(\d+)", hdr).group(1)) == 8
    for dtype, code in hip.FLOW_LOSS_DTYPES.items():
        macro = {torch.float32: "F32", torch.bfloat16: "BF16", torch.float16: "F16"}[dtype]
        assert int(re.search(r"#define\s+SDF_FLOW_LOSS_%s\s+(\d+)" % macro, hdr).group(1)) == code
    assert " flow_loss " in open(os.path.join(ROOT, "sdformerflow_amd", "csrc", "build.sh")).read()
    test_abi_cpu.test_binding_matches_the_header()


def test_every_refusal_comes_before_any_launch():
    """Dummy pointers and no GPU: each call returns its SDF_E_* code without touching them."""
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.lib()
    p = 0x10000
    ws = lib.sdf_flow_loss_workspace_bytes
    assert ws(4, 288, 384, 4) == 4 * (18 * 6) * 4 * 8                                  # one fp64 per (sample, 16 x 64 tile, level)
    assert ws(2, 40, 72, 3) == 2 * (3 * 2) * 3 * 8 and ws(1, 1, 1, 1) == 8
    assert ws(0, 16, 16, 1) == 0 and ws(65536, 16, 16, 1) == 0 and ws(65535, 16, 16, 1) > 0
    assert ws(1, 1 << 15, 1 << 15, 1) == 0 and ws(1, 0, 16, 1) == 0 and ws(1, 16, 0, 1) == 0
    assert ws(1, 16, 16, 0) == 0 and ws(1, 16, 16, 9) == 0 and ws(1, 16, 16, 8) == 8 * 8
    assert lib.sdf_flow_loss_fwd(None, None) == hip.E_NULL

    def fl(levels=((3, 4), (3, 2), (1, 1)), grads=True, **kw):
        """(T, factor) per level below a 32 x 48 frame, B = 2; **kw overrides descriptor members, a tuple value (i, v) one array entry."""
        d = hip.FlowLossDesc()
        d.levels, d.B, d.H, d.W, d.dtype, d.flow_scaling, d.lambda_mod = len(levels), 2, 32, 48, 0, 1.0, 1.0
        d.label = d.mask = d.n_valid = d.loss = d.records = d.workspace = p
        d.workspace_bytes = 1 << 20
        for i, (T, s) in enumerate(levels[:8]):
            d.pred[i], d.h[i], d.w[i], d.T[i] = p, 32 // s, 48 // s, T
            if grads:
                d.grad[i] = p
        for name, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, name)[v[0]] = v[1]
            else:
                setattr(d, name, v)
        return lib.sdf_flow_loss_fwd(C.byref(d), None)
    for member in ("label", "mask", "n_valid", "loss", "workspace"):
        assert fl(**{member: None}) == hip.E_NULL, member
    assert fl(pred=(1, None)) == hip.E_NULL
    assert fl(grad=(2, None)) == hip.E_NULL and fl(grads=False, grad=(1, p)) == hip.E_NULL          # a mix of null and non-null grad
    assert fl(levels=()) == hip.E_SHAPE and fl(levels=((1, 1),) * 9) == hip.E_SHAPE
    assert fl(T=(0, 0)) == hip.E_SHAPE and fl(T=(2, 65)) == hip.E_SHAPE and fl(T=(1, -1)) == hip.E_SHAPE
    assert fl(h=(0, 0)) == hip.E_SHAPE and fl(w=(0, -4)) == hip.E_SHAPE
    assert fl(H=96, W=144, h=(0, 32), w=(0, 48)) == hip.E_SHAPE                                     # factor 3
    assert fl(H=64, W=64, levels=((1, 1),), h=(0, 2), w=(0, 2)) == hip.E_SHAPE                      # factor 32
    assert fl(h=(0, 5)) == hip.E_SHAPE and fl(w=(1, 23)) == hip.E_SHAPE                             # H, W no multiple of the level
    assert fl(h=(0, 16)) == hip.E_SHAPE                                                             # 2 down, 4 across: not square
    assert fl(B=0) == hip.E_SHAPE and fl(B=65536) == hip.E_SHAPE
    assert fl(H=1 << 15, W=1 << 15) == hip.E_SHAPE
    assert fl(workspace_bytes=2 * (2 * 1) * 3 * 8 - 1) == hip.E_SHAPE
    assert fl(dtype=3) == hip.E_DTYPE and fl(dtype=-1) == hip.E_DTYPE
    for member in ("label", "mask", "n_valid", "loss"):
        assert fl(**{member: p + 2}) == hip.E_ALIGN, member
    assert fl(records=p + 4) == hip.E_ALIGN and fl(workspace=p + 4) == hip.E_ALIGN
    assert fl(pred=(0, p + 2)) == hip.E_ALIGN and fl(grad=(1, p + 2)) == hip.E_ALIGN
    assert fl(dtype=1, pred=(0, p + 1)) == hip.E_ALIGN and fl(dtype=2, pred=(2, p + 1)) == hip.E_ALIGN


def test_python_side_refusals():
    from sdformerflow_amd import hip, train
    z = torch.zeros(1, 1, 2, 4, 4)
    with pytest.raises(hip.SdfError):                                                    # CPU tensors: no fallback
        hip.flow_loss([z], torch.zeros(1, 2, 4, 4), torch.ones(1, 4, 4), torch.ones(1))
    with pytest.raises(hip.SdfError, match="levels"):
        hip.flow_loss([], torch.zeros(1, 2, 4, 4), torch.ones(1, 4, 4), torch.ones(1))
    with pytest.raises(hip.SdfError):
        train.flow_loss_hip([z], torch.zeros(1, 2, 4, 4), torch.ones(1, 4, 4))
    with pytest.raises(ValueError, match="head"):
        train.train_step(None, None, None, None, None, head="fused")
    with pytest.raises(ValueError, match="forward_fn"):
        train.train_step(None, None, None, None, None, head="hip", forward_fn=lambda m, x: [])
