"""Host side of the scaled training-step tail (csrc/grad_step.hip: sdf_grad_scale_inplace, sdf_grad_clip_scale_coef,
sdf_adamw_step_scaled), no GPU: the new entry points in the header and the binding; every argument refusal, reported by the library
before any launch; the scale-update restatement against torch.amp.GradScaler on the CPU; LossScaler's state interchange with
GradScaler; the running sum of GradientBuckets.begin(zero=False); train_step's new refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_grad_step_cpu import P, loaded_lib, small_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_grad_scale_inplace", "sdf_grad_clip_scale_coef", "sdf_adamw_step_scaled")


def test_new_entry_points_are_declared_bound_and_built():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    for s in ("SdfLossScaleState", "SdfGradScaleDesc", "SdfGradClipScaleDesc"):
        assert "typedef struct %s" % s in hdr
    assert hip.SIGNATURES["sdf_grad_scale_inplace"] == (C.c_int, (C.POINTER(hip.GradScaleDesc), C.c_void_p))
    assert hip.SIGNATURES["sdf_grad_clip_scale_coef"] == (C.c_int, (C.POINTER(hip.GradClipScaleDesc), C.c_void_p))
    assert hip.SIGNATURES["sdf_adamw_step_scaled"] == (C.c_int, (C.POINTER(hip.AdamwDesc), C.POINTER(hip.LossScaleState), C.c_void_p))
    assert C.sizeof(hip.LossScaleState) == 24 == hip.loss_scale_dtype().itemsize and hip.LossScaleState.skipped.offset == 16
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107         # (additive exports: the version stays)
    lib = loaded_lib()
    assert all(hasattr(lib, n) for n in NEW) and lib.sdf_version() == 107


def scale_rc(lib, pairs=((0, 5), (5, 1), (6, 100)), **kw):
    from sdformerflow_amd import hip
    seg = np.ascontiguousarray(np.array(pairs, dtype=np.int64).reshape(-1, 2))
    d = hip.GradScaleDesc()
    d.flat = d.seg = d.coef = P
    d.seg_host, d.n, d.nseg = seg.ctypes.data, 106, len(seg)
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.sdf_grad_scale_inplace(C.byref(d), None)


def test_grad_scale_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()
    assert lib.sdf_grad_scale_inplace(None, None) == hip.E_NULL
    for f in ("flat", "seg_host", "seg", "coef"):
        assert scale_rc(lib, **{f: None}) == hip.E_NULL, f
    assert scale_rc(lib, mask=None) != hip.E_NULL                                                # no mask: every segment
    assert scale_rc(lib, nseg=0) == hip.E_SHAPE and scale_rc(lib, n=0) == hip.E_SHAPE
    assert scale_rc(lib, pairs=((-1, 5), (5, 1))) == hip.E_SHAPE and scale_rc(lib, pairs=((0, 5), (4, 3))) == hip.E_SHAPE
    assert scale_rc(lib, pairs=((5, 1), (0, 5))) == hip.E_SHAPE and scale_rc(lib, pairs=((0, 5), (5, 0))) == hip.E_SHAPE
    assert scale_rc(lib, pairs=((0, 5), (6, 101))) == hip.E_SHAPE
    assert scale_rc(lib, pairs=((0, 5), ((1 << 62), (1 << 62)))) == hip.E_SHAPE                  # ... without overflowing on the way
    assert scale_rc(lib, flat=P + 2) == hip.E_ALIGN and scale_rc(lib, seg=P + 4) == hip.E_ALIGN and scale_rc(lib, coef=P + 2) == hip.E_ALIGN
    assert scale_rc(lib, flat=P + 4) != hip.E_ALIGN                                              # any float boundary will do
    assert scale_rc(lib, nseg=0, flat=P + 2) == hip.E_SHAPE                                      # the order: shape before alignment
    host = np.full(1 << 12, 3.0, dtype=np.float32)
    keep = host.copy()
    h = host.ctypes.data
    assert scale_rc(lib, flat=h, seg=h, coef=h, mask=h) == hip.E_DTYPE
    assert scale_rc(lib, flat=h + 4, seg=h, coef=h) == hip.E_DTYPE
    assert host.tobytes() == keep.tobytes()


def clip_scale_rc(lib, **kw):
    from sdformerflow_amd import hip
    d = hip.GradClipScaleDesc()
    d.table = d.coef = d.record = d.state = P
    d.rows, d.max_norm, d.growth_factor, d.backoff_factor, d.growth_interval, d.clip_unscaled, d.update = 4, 1.0, 2.0, 0.5, 2000, 0, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.sdf_grad_clip_scale_coef(C.byref(d), None)


def test_grad_clip_scale_coef_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()
    assert lib.sdf_grad_clip_scale_coef(None, None) == hip.E_NULL
    for f in ("table", "coef", "record", "state"):
        assert clip_scale_rc(lib, **{f: None}) == hip.E_NULL, f
    assert clip_scale_rc(lib, rows=0) == hip.E_SHAPE and clip_scale_rc(lib, rows=(1 << 24) + 1) == hip.E_SHAPE
    assert clip_scale_rc(lib, max_norm=-1.0) == hip.E_SHAPE and clip_scale_rc(lib, max_norm=float("nan")) == hip.E_SHAPE
    assert clip_scale_rc(lib, growth_factor=0.0) == hip.E_SHAPE and clip_scale_rc(lib, backoff_factor=float("nan")) == hip.E_SHAPE
    assert clip_scale_rc(lib, growth_interval=0) == hip.E_SHAPE
    assert clip_scale_rc(lib, table=P + 4) == hip.E_ALIGN and clip_scale_rc(lib, record=P + 4) == hip.E_ALIGN
    assert clip_scale_rc(lib, coef=P + 2) == hip.E_ALIGN and clip_scale_rc(lib, state=P + 4) == hip.E_ALIGN
    assert clip_scale_rc(lib, rows=0, state=P + 4) == hip.E_SHAPE
    host = np.full(64, 7.0, dtype=np.float64)
    keep = host.copy()
    h = host.ctypes.data
    for kw in (dict(), dict(max_norm=float("inf")), dict(update=0), dict(clip_unscaled=1), dict(mask=h + 64)):
        assert clip_scale_rc(lib, table=h, coef=h + 256, record=h + 264, state=h + 280, **kw) == hip.E_DTYPE, kw
    assert host.tobytes() == keep.tobytes()


def adamw_scaled_rc(lib, edit=None, state=P, **kw):
    from sdformerflow_amd import hip
    rows = hip.adamw_rows(3)
    rows["param"], rows["offset"], rows["length"], rows["active"] = P, (0, 5, 6), (5, 1, 100), 1
    if edit:
        edit(rows)
    d = hip.AdamwDesc()
    d.grad = d.exp_avg = d.exp_avg_sq = d.rows = P
    d.rows_host, d.n, d.nseg = rows.ctypes.data, 106, 3
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.sdf_adamw_step_scaled(C.byref(d), None if state is None else C.cast(C.c_void_p(state), C.POINTER(hip.LossScaleState)), None)


def test_adamw_step_scaled_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()

    def put(field, i, v):
        def edit(rows):
            rows[field][i] = v
        return edit
    assert lib.sdf_adamw_step_scaled(None, C.cast(C.c_void_p(P), C.POINTER(hip.LossScaleState)), None) == hip.E_NULL
    assert adamw_scaled_rc(lib, state=None) == hip.E_NULL
    for f in ("grad", "exp_avg", "exp_avg_sq", "rows_host", "rows"):
        assert adamw_scaled_rc(lib, **{f: None}) == hip.E_NULL, f
    assert adamw_scaled_rc(lib, put("param", 1, 0)) == hip.E_NULL                            # an active row without its parameter
    assert adamw_scaled_rc(lib, lambda r: (put("param", 1, 0)(r), put("active", 1, 0)(r))) != hip.E_NULL
    assert adamw_scaled_rc(lib, nseg=0) == hip.E_SHAPE and adamw_scaled_rc(lib, nseg=65536) == hip.E_SHAPE
    assert adamw_scaled_rc(lib, put("offset", 0, -1)) == hip.E_SHAPE and adamw_scaled_rc(lib, put("offset", 1, 4)) == hip.E_SHAPE
    assert adamw_scaled_rc(lib, put("length", 1, 0)) == hip.E_SHAPE and adamw_scaled_rc(lib, put("length", 2, 101)) == hip.E_SHAPE
    assert adamw_scaled_rc(lib, n=105) == hip.E_SHAPE
    assert adamw_scaled_rc(lib, grad=P + 2) == hip.E_ALIGN and adamw_scaled_rc(lib, rows=P + 4) == hip.E_ALIGN
    assert adamw_scaled_rc(lib, coef=P + 2) == hip.E_ALIGN and adamw_scaled_rc(lib, state=P + 4) == hip.E_ALIGN
    assert adamw_scaled_rc(lib, exp_avg=P + 4) == hip.E_ALIGN and adamw_scaled_rc(lib, exp_avg_sq=P + 8) == hip.E_ALIGN
    assert adamw_scaled_rc(lib, grad=P + 4, exp_avg=P + 20, exp_avg_sq=P + 36) != hip.E_ALIGN
    assert adamw_scaled_rc(lib, put("param", 2, P + 2)) == hip.E_ALIGN
    assert adamw_scaled_rc(lib, n=105, state=P + 4) == hip.E_SHAPE                           # the order: shape before alignment
    host = np.full(1 << 12, 5.0, dtype=np.float32)
    keep = host.copy()
    h = host.ctypes.data
    assert adamw_scaled_rc(lib, lambda r: r["param"].fill(h), state=h, grad=h, exp_avg=h, exp_avg_sq=h, rows=h, coef=h) == hip.E_DTYPE
    assert host.tobytes() == keep.tobytes()


def test_wrappers_refuse_cpu_tensors():
    from sdformerflow_amd import hip
    z = torch.zeros(16)
    state = hip.loss_scale_state(device="cpu")
    assert hip.loss_scale_read(state) == {"scale": 65536.0, "growth_tracker": 0, "inv_scale": 2.0 ** -16, "found_inf": 0, "skipped": 0}
    with pytest.raises(hip.SdfError):
        hip.grad_scale(z, [(0, 16)], torch.ones(1))
    with pytest.raises(hip.SdfError):
        hip.grad_clip_scale_coef(torch.zeros(2, 5, dtype=torch.float64), 1.0, state)
    with pytest.raises(hip.SdfError):
        hip.adamw_step_scaled(z, z.clone(), z.clone(), hip.adamw_rows(1), state)
    assert not z.any() and hip.loss_scale_read(state)["skipped"] == 0


# ------------------------------------------------------------------------------------------------ the scale update
# (found_inf per step) with growth_interval 2 from 2^126: growth to 2^127, a growth that would overflow to inf (refused, tracker
# back to 0), a non-finite step (backoff), growth again, two non-finite steps in a row, growth
TRAJECTORY = (0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0)


def torch_scaler_trajectory(device, init_scale, found, **kw):
    """[(scale, tracker)] of torch.amp.GradScaler after each step of `found` (1: a gradient is inf)."""
    p = torch.nn.Parameter(torch.zeros(3, device=device))
    opt = torch.optim.SGD([p], lr=0.0)
    gs = torch.amp.GradScaler(device, init_scale=init_scale, **kw)
    out = []
    for f in found:
        gs.scale(torch.zeros((), device=device))
        p.grad = torch.tensor([1.0, float("inf") if f else 2.0, 3.0], device=device)
        gs.step(opt)
        gs.update()
        out.append((gs.get_scale(), int(gs._growth_tracker)))
    return out


@pytest.mark.parametrize("init,growth,backoff,interval", [(2.0 ** 126, 2.0, 0.5, 2), (65536.0, 2.0, 0.5, 2), (1000.0, 1.5, 0.75, 3)])
def test_scale_restatement_matches_torch_grad_scaler(init, growth, backoff, interval):
    from sdformerflow_amd import train
    want = torch_scaler_trajectory("cpu", init, TRAJECTORY, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    scale, tracker, seen = init, 0, set()
    for f, (w_scale, w_tracker) in zip(TRAJECTORY, want):
        new = train.loss_scale_restatement(scale, tracker, f, growth, backoff, interval)
        seen.add("backoff" if f else "overflow" if tracker + 1 == interval and new[0] == scale else "growth" if new[0] > scale else "count")
        scale, tracker = new
        assert (scale, tracker) == (w_scale, w_tracker), (f, scale, tracker, w_scale, w_tracker)
    assert {"backoff", "growth", "count"} <= seen and (("overflow" in seen) == (init == 2.0 ** 126))


def test_loss_scaler_state_interchanges_with_torch_grad_scaler():
    from sdformerflow_amd import train
    ours = train.LossScaler(init_scale=1024.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7, device="cpu")
    assert list(ours.state_dict()) == list(torch.amp.GradScaler("cpu").state_dict())
    ours._views["growth_tracker"].fill_(5)
    # ours -> torch
    gs = torch.amp.GradScaler("cpu")
    gs.load_state_dict(ours.state_dict())
    assert gs.state_dict() == ours.state_dict() == {"scale": 1024.0, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 7,
                                                     "_growth_tracker": 5}
    # torch -> ours, from a scaler that has stepped
    want = torch_scaler_trajectory("cpu", 64.0, (0, 0, 1, 0), growth_factor=2.0, backoff_factor=0.5, growth_interval=2)[-1]
    gs = torch.amp.GradScaler("cpu", init_scale=64.0, growth_interval=2)
    gs.scale(torch.zeros(()))
    gs._scale.fill_(want[0])
    gs._growth_tracker.fill_(want[1])
    ours.load_state_dict(gs.state_dict())
    assert ours.state_dict() == gs.state_dict() and ours.get_scale() == want[0] == 64.0 and ours.growth_interval == 2
    from sdformerflow_amd import hip
    assert hip.loss_scale_read(ours.state)["inv_scale"] == 1.0 / 64.0
    assert float(ours.scale(torch.tensor(0.5))) == 32.0
    # a disabled scaler: scale 1, the loss is handed back, GradScaler's empty state
    off = train.LossScaler(enabled=False, device="cpu")
    loss = torch.tensor(0.5)
    assert off.get_scale() == 1.0 and off.scale(loss) is loss and off.state_dict() == torch.amp.GradScaler("cpu", enabled=False).state_dict() == {}
    with pytest.raises(ValueError):
        train.LossScaler(growth_factor=1.0, device="cpu")
    with pytest.raises(RuntimeError):
        ours.load_state_dict({})


def test_buckets_keep_the_running_sum_when_asked():
    from sdformerflow_amd import train
    net = small_net()
    buckets = train.GradientBuckets(net.parameters())
    x = torch.randn(4, 5, generator=torch.Generator().manual_seed(1))
    sums = None
    for k in range(3):
        buckets.begin(zero=(k == 0))
        net(x * (k + 1)).sum().backward()
        buckets.finish()
        g = [p.grad.clone() for p in net.parameters()]
        sums = g if sums is None else sums
        assert all(p.grad.data_ptr() == buckets._views[p].data_ptr() for p in net.parameters())
    twin = small_net()
    for k in range(3):
        twin(x * (k + 1)).sum().backward()
    assert all(torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-6) for a, b in zip(net.parameters(), twin.parameters()))
    # a parameter that received a gradient in an earlier micro-step only keeps it
    buckets.begin()
    net(x).sum().backward()
    buckets.finish()
    buckets.begin(zero=False)
    net[1](torch.randn(2, 7)).sum().backward()
    buckets.finish()
    assert all(p.grad is not None for p in net.parameters())
    buckets.begin()                                                          # ... until the buckets are zeroed
    net[1](torch.randn(2, 7)).sum().backward()
    buckets.finish()
    assert net[0].weight.grad is None and net[1].weight.grad is not None


def test_train_step_refuses_what_the_scaled_tail_cannot_serve():
    from sdformerflow_amd import train
    net = small_net()
    buckets = train.GradientBuckets(net.parameters())
    opt = train.BucketAdamW(buckets, 1e-3)
    stock = torch.optim.AdamW(net.parameters())
    scaler = train.LossScaler(device="cpu")
    with pytest.raises(NotImplementedError, match="use train.BucketAdamW"):
        train.train_step(net, stock, None, None, None, buckets=buckets, scaler=scaler)
    with pytest.raises(NotImplementedError, match="use train.BucketAdamW"):
        train.train_step(net, stock, None, None, None, buckets=buckets, num_acc=2)
    with pytest.raises(NotImplementedError, match="accumulate on one rank"):
        train.train_step(net, opt, None, None, None, buckets=buckets, num_acc=2, dist=object(), world=2)
    with pytest.raises(ValueError, match="needs a loss scaler"):
        train.train_step(net, opt, None, None, None, buckets=buckets, amp="fp16")
    with pytest.raises(TypeError, match="train.LossScaler"):
        train.train_step(net, opt, None, None, None, buckets=buckets, amp="fp16", scaler=torch.amp.GradScaler("cpu"))
    with pytest.raises(ValueError, match="amp is"):
        train.train_step(net, opt, None, None, None, buckets=buckets, amp="fp8")
    with pytest.raises(ValueError, match="pass scaler="):
        train.get_grads(net, buckets, unscale=True)
    from sdformerflow_amd import hip
    with pytest.raises(hip.SdfError, match="lives on the GPU"):
        opt.step(1.0, scaler=scaler)                                         # a host-resident state never reaches a launch
    from test_ann_model import build
    ann = build()
    ab = train.GradientBuckets(ann.parameters())
    with pytest.raises(NotImplementedError, match="pass amp=False"):
        train.train_step(ann, train.BucketAdamW(ab, 1e-3), None, None, None, buckets=ab, amp="fp16", scaler=scaler, clip_grad=None)
    assert all(float(opt.state[p]["step"]) == 0.0 for p in buckets.params) and scaler.state_dict()["scale"] == 65536.0
