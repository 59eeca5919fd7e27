"""hip.flow_loss (csrc/flow_loss.hip) and train_step(head="hip") against the torch head - forward_train's sum over time and nearest
upsampling followed by train.flow_loss_supervised, fp32 on the GPU - and against the fp64 restatement of tests/test_flow_loss_cpu.py.

The value bound is the project's 2 d rule.  With d the distance of the torch composition from the fp64 restatement (per tensor, largest
element), the kernel's distance from the restatement is at most max(2 d, c * 2^-24 * A) at every element, A being the restatement of
the same expression with every term replaced by its absolute value (|f fs| + |label| in place of the difference; a gradient element:
summed over its s x s block) and c the number of rounded fp32 operations on the element's path:
  a record S[i][b]: per pixel 2 (T - 1) additions over time, 2 products with flow_scaling, 2 subtractions, 2 squares, 2 additions (the
      sum and the 1e-8), the root and the product with the mask: c = 2 (T - 1) + 10; the sum itself is fp64.
  the loss: the same, + the fp32 n + 1e-9 and the one rounding of the result: c = 2 (T - 1) + 12.
  a gradient element: the root's path without the mask, 2 (T - 1) + 9; m * d, / r, * k: 3; k itself (the fp32 constant, n + 1e-9, the
      division): 3; the block's s^2 - 1 additions: c = s^2 + 2 (T - 1) + 14.
Shapes: the smallest with a partial column tile, a partial row tile, the largest factor and the T = 1 form; every case has pixels where
pred * fs == label exactly, and (B > 1) a sample whose mask is all zero."""
import functools

import numpy as np
import pytest
import torch

from sdformerflow_amd import hip, train
from test_flow_loss_cpu import restate64
from test_grad_step_gpu import DEV, carve, deterministic_convolutions, guarded, guards_intact, kname  # noqa: F401  (a fixture among them)

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
FS, LAM = 1.5, 0.75
# (B, T, H, W, factors)
CASES = {"column_tile": (2, 3, 48, 80, (8, 4, 2, 1)), "row_tile": (2, 1, 40, 72, (8, 4, 2, 1)), "factor16": (1, 2, 32, 48, (16,)),
         "ann": (3, 1, 24, 40, (1,))}
RUNS = [(c, torch.float32) for c in CASES] + [("column_tile", torch.bfloat16), ("column_tile", torch.float16)]
IDS = [f"{c}-{str(t).split('.')[-1]}" for c, t in RUNS]


def make_inputs(case, dtype, seed=7):
    """(preds, label, mask, n) on the CPU: normal draws; quarters in a strip of the finest level, where the label is made equal to
    pred.sum(0) * FS exactly (exact in every dtype); a 0 / 1 mask, all zero in the last sample of a batch."""
    B, T, H, W, factors = CASES[case]
    g = torch.Generator().manual_seed(seed)
    preds = [torch.randn((T, B, 2, H // s, W // s), generator=g) for s in factors]
    s = factors[-1]
    preds[-1][..., 1, 0:2] = torch.round(preds[-1][..., 1, 0:2] * 4) / 4
    preds = [p.to(dtype) for p in preds]
    label = torch.randn((B, 2, H, W), generator=g) * 2
    hit = (preds[-1].float().sum(0) * FS)[..., 1:2, 0:2].repeat_interleave(s, -2).repeat_interleave(s, -1)
    label[:, :, s:2 * s, 0:2 * s] = hit
    mask = (torch.rand((B, 1, H, W), generator=g) < 0.7).float()
    mask[:, :, s:2 * s, 0:2 * s] = 1.0
    if B > 1:
        mask[-1] = 0.0
    return preds, label, mask, mask.sum()


def run_kernel(preds, label, mask, n, grads=True, records=True):
    """hip.flow_loss with loss, gradients and records in windows between guard bytes.  Returns (loss, grads or None, records or None)."""
    B, L = label.shape[0], len(preds)
    windows = []

    def window(dtype, shape):
        count = int(np.prod(shape))
        nbytes = count * torch.empty(0, dtype=dtype).element_size()
        outer, off = guarded(nbytes)
        windows.append((outer, off, nbytes))
        return carve(outer, off, dtype, count).view(shape)
    loss = window(torch.float32, (1,))
    gs = [window(torch.float32, (B, 2) + tuple(p.shape[-2:])) for p in preds] if grads else False
    rec = window(torch.float64, (L, B)) if records else None
    out, got = hip.flow_loss(preds, label, mask, n, FS, LAM, grads=gs, records=rec, loss=loss)
    torch.cuda.synchronize()
    assert all(guards_intact(*w) for w in windows)
    assert out.data_ptr() == loss.data_ptr() and (got is None if not grads else all(a is b for a, b in zip(got, gs)))
    return out.clone(), ([g.clone() for g in got] if grads else None), (rec.clone() if records else None)


def torch_head(preds, label, mask, n):
    """The torch composition on the GPU, fp32 behind the predictions' dtype as train_step runs it: (loss, [d loss / d preds[i].sum(0)],
    records (levels, B))."""
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    flows = [f.float() for f in train._flows_of_preds(leaves, *label.shape[-2:])]
    loss = train.flow_loss_supervised(flows, label, mask, FS, LAM, n_valid=n)
    loss.backward()
    B = label.shape[0]
    with torch.no_grad():
        rec = torch.stack([(torch.sqrt((f * FS - label).pow(2).sum(1) + 1e-8).view(B, -1) * mask.reshape(B, -1)).sum(1) for f in flows])
    assert all(torch.allclose(p.grad[0], p.grad[-1], rtol=0, atol=0, equal_nan=True) for p in leaves)
    return loss.detach(), [p.grad[0].float() for p in leaves], rec


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """Inputs on the device, the restatement and the torch head of a run - computed once, shared by the tests, never written to."""
    preds, label, mask, n = make_inputs(case, dtype)
    r = restate64(preds, label, mask, float(n), FS, LAM)
    dev = [p.to(DEV) for p in preds], label.to(DEV), mask.to(DEV), n.to(DEV).reshape(1)
    return dev, r, torch_head(*dev)


def counts(case):
    B, T, H, W, factors = CASES[case]
    return 2 * (T - 1) + 12, 2 * (T - 1) + 10, [s * s + 2 * (T - 1) + 14 for s in factors]


def same_classes(got, want):
    """finite / NaN / +-inf and exact zeros at the same elements"""
    return (torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isposinf(got), torch.isposinf(want))
            and torch.equal(torch.isneginf(got), torch.isneginf(want)) and torch.equal(got == 0, want == 0))


@pytest.mark.parametrize("case,dtype", RUNS, ids=IDS)
def test_values_obey_the_2d_rule(case, dtype):
    (preds, label, mask, n), r, (t_loss, t_grads, t_rec) = reference(case, dtype)
    loss, grads, rec = run_kernel(preds, label, mask, n)
    c_loss, c_rec, c_grads = counts(case)
    d = abs(float(t_loss) - r["loss"])
    err = abs(float(loss) - r["loss"])
    print(f"{case} {dtype}: loss {float(loss)!r} (torch {float(t_loss)!r}, fp64 {r['loss']!r}): d {d:.3e}, kernel {err:.3e}, "
          f"c u A {c_loss * U24 * r['A_loss']:.3e}")
    assert err <= max(2 * d, c_loss * U24 * r["A_loss"])
    d = float((t_rec.cpu().double() - r["records"]).abs().max())
    err = (rec.cpu() - r["records"]).abs()
    print(f"  records: d {d:.3e}, kernel {float(err.max()):.3e}")
    assert bool((err <= torch.clamp(c_rec * U24 * r["A_records"], min=2 * d)).all())
    for i, (g, tg) in enumerate(zip(grads, t_grads)):
        assert g.dtype == torch.float32 and g.shape == r["grads"][i].shape
        d = float((tg.cpu().double() - r["grads"][i]).abs().max())
        err = (g.cpu().double() - r["grads"][i]).abs()
        print(f"  level {i} (factor {CASES[case][4][i]}): d {d:.3e}, kernel {float(err.max()):.3e}, largest |g| {float(r['grads'][i].abs().max()):.3e}")
        assert bool((err <= torch.clamp(c_grads[i] * U24 * r["A_grads"][i], min=2 * d)).all()), i
        assert dtype != torch.float32 or same_classes(g, tg), i          # (a 16-bit torch gradient is rounded, and may underflow, in 16 bits)
    assert bool((grads[-1][:, :, 1, 0:2] == 0).all())                     # pred * fs == label over the whole block: an exact zero
    if label.shape[0] > 1:
        assert all(not g[-1].any() for g in grads) and not rec[:, -1].any()                  # the sample with the all-zero mask


@pytest.mark.parametrize("case,dtype", RUNS[:3] + RUNS[4:5], ids=IDS[:3] + IDS[4:5])
def test_two_runs_give_the_same_bytes_and_a_sample_depends_on_itself_alone(case, dtype):
    (preds, label, mask, n), _, _ = reference(case, dtype)
    first, again = run_kernel(preds, label, mask, n), run_kernel(preds, label, mask, n)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first[1], again[1]))
    assert torch.equal(first[2].view(torch.int64), again[2].view(torch.int64))
    only_loss = run_kernel(preds, label, mask, n, grads=False)
    assert torch.equal(only_loss[0], first[0]) and torch.equal(only_loss[2], first[2])
    for b in range(label.shape[0]):                                       # alone, with the batch's n
        _, _, rec = run_kernel([p[:, b:b + 1] for p in preds], label[b:b + 1], mask[b:b + 1], n, grads=False)
        assert torch.equal(rec[:, 0].view(torch.int64), first[2][:, b].view(torch.int64)), b


def test_two_launches_whatever_the_number_of_levels():
    """The forward is the partial and the finish kernel for one level and for four, with gradients and without (`grads=False` writes
    and returns none); autograd's backward through FlowLossFunction launches nothing of the library."""
    (preds, label, mask, n), _, _ = reference("column_tile", torch.float32)
    two = ["flow_loss_partial_kernel", "flow_loss_finish_kernel"]
    for levels, grads in ((preds, True), (preds[:1], True), (preds, False), (preds[2:], False)):
        with hip.launch_log() as log:
            _, got = hip.flow_loss(levels, label, mask, n, FS, LAM, grads=grads)
        assert [kname(r[0]) for r in log.rows] == two and (got is None) == (not grads)
        assert log.rows[0][1:3] == (3 * 2 * label.shape[0], 256) and log.rows[1][1:3] == (1, 256)
    leaves = [p.clone().requires_grad_(True) for p in preds]
    with hip.launch_log() as log:
        loss = train.flow_loss_hip(leaves, label, mask, FS, LAM, n_valid=n)
    assert [kname(r[0]) for r in log.rows] == two
    with hip.launch_log() as log:
        (loss * 3.0).backward()
    assert log.rows == []
    _, grads = hip.flow_loss(preds, label, mask, n, FS, LAM)
    for leaf, g in zip(leaves, grads):
        assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad[0], g * 3.0) and torch.equal(leaf.grad[0], leaf.grad[-1])
    with torch.no_grad(), hip.launch_log() as log:
        quiet = train.flow_loss_hip(leaves, label, mask, FS, LAM, n_valid=n)
    assert [kname(r[0]) for r in log.rows] == two and not quiet.requires_grad and torch.equal(quiet, loss.detach())


@pytest.mark.parametrize("case", ["column_tile", "factor16"])
def test_edge_semantics_are_torchs(case):
    (preds, label, mask, n), _, _ = reference(case, torch.float32)
    B, T, H, W, factors = CASES[case]
    # no valid pixel at all, n = 0: loss 0 and zero gradients
    zero_mask, zero = torch.zeros_like(mask), torch.zeros(1, device=DEV)
    loss, grads, _ = run_kernel(preds, label, zero_mask, zero)
    t_loss, t_grads, _ = torch_head(preds, label, zero_mask, zero)
    assert float(loss) == 0.0 and float(t_loss) == 0.0 and all(not g.any() for g in grads) and all(not g.any() for g in t_grads)
    # an inf in the coarsest prediction, at a valid pixel and at a masked one
    s = factors[0]
    for valid in (True, False):
        m = mask.clone()
        m[0, :, s:2 * s, 2 * s:3 * s] = float(valid)                     # the frame under pixel (1, 2) of the coarsest level
        bad = [p.clone() for p in preds]
        bad[0][T - 1, 0, 1, 1, 2] = float("inf")
        nn = m.sum().reshape(1)
        loss, grads, rec = run_kernel(bad, label, m, nn)
        t_loss, t_grads, t_rec = torch_head(bad, label, m, nn)
        print(f"{case}, inf at a {'valid' if valid else 'masked'} pixel: loss {float(loss)} (torch {float(t_loss)}), gradient element "
              f"{float(grads[0][0, 1, 1, 2])} (torch {float(t_grads[0][0, 1, 1, 2])})")
        assert not torch.isfinite(loss) and same_classes(loss.reshape(()), t_loss.reshape(()))
        assert bool(torch.isnan(loss)) == (not valid)
        assert not torch.isfinite(grads[0][0, 1, 1, 2])
        assert same_classes(rec.float(), t_rec)
        for g, tg in zip(grads, t_grads):
            assert same_classes(g, tg)


# ------------------------------------------------------------------------------------------------ the step
def bucket_grads(buckets):
    return {p: buckets._views[p].detach().clone() for p in buckets.params if p.grad is not None}


def test_train_step_heads_agree(deterministic_convolutions):
    """One model (3 encoders, 144 x 144, batch 2), three passes from the same weights under an SGD of rate 0: head="torch", head="hip",
    and the torch head computed in fp64 from the same raw predictions.  The forwards are the same launches; the loss obeys the bound of
    test_values_obey_the_2d_rule, and every parameter's gradient of the hip head lies within 2 d of the torch head's, d the distance of
    the torch head's gradient from the fp64 head's (floor: one ulp of the gradient's largest element).  The default head logs no
    flow_loss kernel; the hip head exactly its two."""
    from sdformerflow_amd.spikingjelly_compat import functional
    from test_train_gpu import small_model
    model, chunk, label, mask = small_model()
    names = {p: n for n, p in model.named_parameters()}
    buckets = train.GradientBuckets(model.parameters())
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    with hip.launch_log() as log:
        t_loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=None)
    assert log.rows and not any("flow_loss" in r[0] for r in log.rows)
    g_torch = bucket_grads(buckets)
    with hip.launch_log() as log:
        h_loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=None, head="hip")
    kernels = [kname(r[0]) for r in log.rows]
    assert [k for k in kernels if "flow_loss" in k] == ["flow_loss_partial_kernel", "flow_loss_finish_kernel"]
    g_hip = bucket_grads(buckets)
    # the fp64 head on the same predictions, back-propagated through the same model
    model.train()
    functional.reset_net(model)
    buckets.begin()
    preds = train.forward_train_preds(model, chunk)
    n = train.global_valid_count(mask)
    flows = train._flows_of_preds([p.double() for p in preds], *chunk.shape[-2:])
    train.flow_loss_supervised(flows, label.double(), mask.double(), 1.0, 1.0, n_valid=n.double()).backward()
    buckets.finish()
    g_64 = bucket_grads(buckets)
    assert list(g_torch) == list(g_hip) == list(g_64) and len(g_torch) > 200

    T = preds[0].shape[0]
    r = restate64([p.detach() for p in preds], label, mask, float(n), 1.0, 1.0)
    d, err = abs(float(t_loss) - r["loss"]), abs(float(h_loss) - r["loss"])
    print(f"loss: hip {float(h_loss)!r}, torch {float(t_loss)!r}, fp64 {r['loss']!r}: d {d:.3e}, hip head {err:.3e}")
    assert err <= max(2 * d, (2 * (T - 1) + 12) * U24 * r["A_loss"])
    worst = (0.0, None)
    for p, gt in g_torch.items():
        d = float((gt.double() - g_64[p].double()).abs().max())
        e = float((g_hip[p].double() - gt.double()).abs().max())
        ulp = float(np.spacing(np.float32(gt.abs().max().item())))
        worst = max(worst, (e / max(2 * d, ulp), names[p]))
        print(f"  {names[p]}: d {d:.3e}, hip - torch {e:.3e}, ulp {ulp:.3e}")
        assert e <= max(2 * d, ulp), (names[p], e, d, ulp)
    print(f"worst ratio to the bound {worst[0]:.3f} ({worst[1]})")


def test_fp16_step_heads_agree_on_skip_and_scale(deterministic_convolutions):
    """amp="fp16" with a LossScaler and BucketAdamW, one step per head from the same weights: the same verdict (skip or step), the same
    scale and growth count afterwards, finite parameters."""
    from test_train_gpu import small_model
    verdicts = {}
    for head in ("torch", "hip"):
        model, chunk, label, mask = small_model()
        buckets = train.GradientBuckets(model.parameters())
        opt = train.BucketAdamW(buckets, 1e-3, weight_decay=0.01)
        scaler = train.LossScaler(init_scale=65536.0, device=DEV)
        loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=100.0, amp="fp16", scaler=scaler, head=head)
        st = hip.loss_scale_read(scaler.state)
        verdicts[head] = (bool(st["found_inf"]), st["scale"], st["growth_tracker"])
        print(f"head {head}: loss {float(loss)!r}, skipped {verdicts[head][0]}, scale afterwards {st['scale']}")
        assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in model.parameters())
    assert verdicts["torch"] == verdicts["hip"]


def test_sew_model_steps_with_the_hip_head():
    from test_sew_train_gpu import small_model as sew_model
    model, chunk, label, mask, _ = sew_model()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    with hip.launch_log() as log:
        loss = train.train_step(model, opt, chunk, label, mask, head="hip")
    assert sum("flow_loss" in r[0] for r in log.rows) == 2
    assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in model.parameters())


def test_ann_model_steps_with_the_hip_head():
    """An STTFlowNet's full-resolution flows are factor-1 levels of one time step."""
    import os
    from test_ann_train_gpu import ROOT, build
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    B, BINS, H, W, SEED = (int(v) for v in np.load(os.path.join(ROOT, "tests", "golden", "ann_train_step.npz"))["cfg"])
    net = build((H, W))
    vox = synth_voxel(B, BINS, H, W, seed=SEED).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=SEED + 1))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4)
    with hip.launch_log() as log:
        loss = train.train_step(net, opt, vox, label, mask, clip_grad=None, head="hip")
    assert sum("flow_loss" in r[0] for r in log.rows) == 2
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p).all() for p in net.parameters())
