"""Training with PLIF neurons (spikingjelly ParametricLIFNode, `neuron_type: plif`) on the GPU: the HIP forward / BPTT kernels
with dL/dk (csrc/neuron.hip, csrc/neuron_bwd.hip) and the fused PLIF token gate (csrc/qk_gate_train.hip) against fixtures made by
the REAL reference's autograd (tests/golden/make_golden_plif_train.py), against the LIF path at the neutral k = 0.5, against the
composed gate expression; a train step, the engine rebuild after it, and the absence of host synchronisation."""
import os

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import hip, train
from sdformerflow_amd.autograd import PLIFFunction, QKGatePLIFFunction
from sdformerflow_amd.STSwinNet_SNN import Spiking_swin_transformer3D as SW
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import ParametricLIFNode
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_uniform as rnd, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
PG = np.load(os.path.join(HERE, "golden", "plif_grads.npz"))
PB = np.load(os.path.join(HERE, "golden", "plif_train_block.npz"))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
RESETS = {"soft": None, "hard": 0.0, "hard005": 0.05}


def charge_differences(x, k, v_th, v_reset):
    """d_t of the forward (the reference's op order, fp32 on the host): what dL/dk sums gh against."""
    v = torch.full_like(x[0], 0.0 if v_reset is None else v_reset)
    ds = []
    for t in range(x.shape[0]):
        d = x[t] - v if v_reset in (None, 0.0) else x[t] - (v - v_reset)
        h = v + d * k
        s = (h - v_th >= 0).float()
        v = h - s * v_th if v_reset is None else (1.0 - s) * h + s * v_reset
        ds.append(d)
    return torch.stack(ds)


@pytest.mark.parametrize("T", [2, 4, 10])
@pytest.mark.parametrize("tag", ["soft", "hard", "hard005"])
@pytest.mark.parametrize("detach", [True, False])
def test_plif_kernels_match_reference_autograd(T, tag, detach):
    key = f"{tag}_{'detach' if detach else 'nodetach'}_T{T}"
    v_th, v_reset = float(PG["v_th"]), RESETS[tag]
    N = PG[f"{key}_gx"].shape[1]
    x0 = rnd((T, N), 500 + T, -0.3, 0.6)                             # the generator's inputs, from its seeds
    x0[:, :64] = 0.1
    assert int(PG[f"{tag}_T{T}_ties"]) > 0                        # h == v_th exactly at t = 0 in these columns
    x0[0, 64:128] = float(PG[f"{tag}_T{T}_tie_x"])
    g = rnd((T, N), 600 + T, -1.0, 2.0)
    w = torch.tensor(float(PG["w"]), device=DEV, requires_grad=True)
    x = x0.to(DEV).requires_grad_(True)
    s = PLIFFunction.apply(x, torch.sigmoid(w), v_th, v_reset, detach, 2.0)
    s.backward(g.to(DEV))
    assert torch.equal(s.detach().to(torch.uint8).cpu(), torch.from_numpy(PG[f"{key}_s"]))
    gx_ref = torch.from_numpy(PG[f"{key}_gx"])
    if detach:
        assert torch.equal(x.grad.cpu(), gx_ref)
    else:
        assert (x.grad.cpu() - gx_ref).abs().max().item() <= 1e-6 * gx_ref.abs().max().item()
    k = torch.sigmoid(torch.tensor(float(PG["w"])))
    d = charge_differences(x0, k, v_th, v_reset)
    scale = float((gx_ref / k * d).abs().sum() * k * (1 - k))        # sum |gh d| carried to w
    gw_ref = float(PG[f"{key}_gw"])
    assert abs(w.grad.item() - gw_ref) <= 1e-5 * scale, (w.grad.item(), gw_ref, scale)
    # two backward calls: bit-equal dL/dx and dL/dk (fixed-order reduction)
    kd = torch.sigmoid(w.detach()).reshape(1)
    a = hip.plif_bwd(x.detach(), kd, g.to(DEV), v_th, v_reset, detach, 2.0)
    b = hip.plif_bwd(x.detach(), kd, g.to(DEV), v_th, v_reset, detach, 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_plif_forward_matches_the_eval_engine_and_an_odd_size():
    """Train-mode spikes are the eval path's spikes for the same k (sdf_lif_fwd with tau = k), also at N % 4 != 0."""
    x = rnd((10, 3 * 1001), 77, -0.3, 0.6).to(DEV)
    for w in (0.35, -1.2):
        k = torch.sigmoid(torch.tensor(w, device=DEV))
        for v_reset in (None, 0.05):
            got = hip.plif_fwd(x, k.reshape(1), 0.1, v_reset)
            want = hip.lif_fwd(x, float(k), 0.1, v_reset)
            assert torch.equal(got, want)


def kw(kind, T):
    return {"num_steps": T, "v_reset": None, "v_th": 0.1, "neuron_type": kind, "surrogate_fun": "surrogate.ATan()", "tau": 2.0,
            "detach_reset": True, "spike_norm": "BN"}


def rate(got, ref):
    got, ref = got.detach().float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape
    scale = ref.abs().mean().item() + 1e-12
    return ((got - ref).abs() > 1e-3 * scale).float().mean().item()


def picked(t, key):
    """The elements of t the fixture kept under `key` (all of them, or those at `key@idx`), flattened."""
    t = t.detach().reshape(-1)
    return t[torch.from_numpy(PB[key + "@idx"]).long().to(t.device)] if key + "@idx" in PB.files else t


def test_plif_train_mode_block_matches_reference_autograd():
    """Mismatch rates over the elements the fixture kept (a seeded random sample of the large tensors)."""
    B, H, W, *shift = (int(v) for v in PB["cfg"])
    blk = SW.MS_Spiking_SwinTransformerBlock3D(96, (H, W), 3, window_size=(2, 9, 9), shift_size=tuple(shift), norm_layer="BN",
                                               **kw("plif", 4))
    blk.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}), strict=True)
    with torch.no_grad():
        for k in PB.files:
            if k.startswith("w/"):
                blk.get_parameter(k[2:]).copy_(torch.from_numpy(PB[k]))
    blk = blk.to(DEV).train()
    x = rnd((B, 4, H, W, 96), 17, -0.5, 1.0).to(DEV).requires_grad_(True)
    g = rnd((B, 4, H, W, 96), 18, -1.0, 2.0).to(DEV)
    y = train.ms_block(x, blk, training=True)
    y.backward(g)
    report = {"y": rate(picked(y, "y"), PB["y"]), "gx": rate(picked(x.grad, "gx"), PB["gx"])}
    params = dict(blk.named_parameters())
    nodes = 0
    for k in PB.files:
        if not k.startswith("g/") or k.endswith("@idx"):
            continue
        name = k[2:]
        if name.endswith("spiking_neuron.w"):
            ref = float(PB[k].reshape(-1)[0])                       # (stored flattened, one element)
            assert abs(params[name].grad.item() - ref) <= 1e-3 * abs(ref), (name, params[name].grad.item(), ref)
            nodes += 1
        elif name.endswith("proj.bias"):
            assert params[name].grad.abs().max().item() < 1e-3 * float(np.abs(PB["g/attn.proj.weight"]).mean())
        else:
            report[name] = rate(picked(params[name].grad, k), PB[k])
    for k in PB.files:
        if k.startswith("r/"):
            report["running:" + k[2:]] = rate(picked(dict(blk.named_buffers())[k[2:]], k), PB[k])
    assert nodes == 6                                                 # sn_q, sn_k, sn2_q (the gate), proj_sn, mlp.sn1, mlp.sn2
    worst = max(report.values())
    print(f"plif train block: mismatch rates y {report['y']:.2e} gx {report['gx']:.2e} worst {worst:.2e}")
    assert report["y"] <= 2e-3 and report["gx"] <= 5e-3 and worst <= 1e-2, report


@pytest.mark.parametrize("Tq", [1, 2, 4])
@pytest.mark.parametrize("Cc", [96, 192])
def test_fused_plif_gate_equals_the_composed_expression(Tq, Cc):
    """(dq, dk, dk_gate) of QKGatePLIFFunction against PLIFFunction on the per-head sums -> repeat_interleave -> multiply.  dL/de holds
    multiples of 1/16, so the per-head sums of dL/de * k are exact in any order and dq, dk are compared at 1e-6 of the largest
    element; dL/dk_gate is a sum over (t, row, head) in two different fixed orders: 1e-6 of sum |gh d| (carried to w)."""
    rows, nH = 2 * 81 + 5, Cc // 32
    gen = torch.Generator().manual_seed(Tq * 1000 + Cc)
    q = (torch.rand((Tq, rows, Cc), generator=gen) < 0.35).float().to(DEV)
    kk = (torch.rand((Tq, rows, Cc), generator=gen) < 0.3).float().to(DEV)
    ge = (torch.randint(-64, 65, (Tq, rows, Cc), generator=gen).float() / 16).to(DEV)
    for v_th, v_reset, detach in ((5.0, None, True), (6.0, 0.0, False), (5.0, 0.05, False)):
        w1 = torch.tensor(0.35, device=DEV, requires_grad=True)
        q1, k1 = q.clone().requires_grad_(True), kk.clone().requires_grad_(True)
        QKGatePLIFFunction.apply(q1, k1, torch.sigmoid(w1), v_th, v_reset, detach, 2.0).backward(ge)
        w2 = torch.tensor(0.35, device=DEV, requires_grad=True)
        q2, k2 = q.clone().requires_grad_(True), kk.clone().requires_grad_(True)
        sums = q2.reshape(Tq, rows, nH, 32).sum(-1)
        sums.retain_grad()
        a = PLIFFunction.apply(sums, torch.sigmoid(w2), v_th, v_reset, detach, 2.0)
        (k2 * a.repeat_interleave(32, dim=-1)).backward(ge)
        for got, want in ((q1.grad, q2.grad), (k1.grad, k2.grad)):
            assert (got - want).abs().max().item() <= 1e-6 * want.abs().max().item(), (v_th, v_reset, detach)
        k = torch.sigmoid(torch.tensor(0.35))
        gh, d = sums.grad.cpu() / k, charge_differences(sums.detach().cpu(), k, v_th, v_reset)
        scale = float((gh * d).abs().sum() * k * (1 - k))
        assert abs(w1.grad.item() - w2.grad.item()) <= 1e-6 * scale, (w1.grad.item(), w2.grad.item(), scale)
        assert w1.grad.item() != 0.0


def small_kwargs(cfg, kind):
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"].update(input_size=[144, 144], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    return cfg["model"].copy(), cfg["swin_transformer"].copy()


def small_model(kind, w=0.0):
    """The 3-encoder model of test_train_gpu.small_model; PLIF nodes get w (0: k = 0.5 exactly, LIF tau = 2)."""
    model = MS_SpikingformerFlowNet(*small_kwargs(yaml.safe_load(open(CFG)), kind))
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, ParametricLIFNode):
                m.w.fill_(w)
    model = model.to(DEV).train()
    for m in model.modules():
        if hasattr(m, "drop_path_rate"):
            m.drop_path_rate = 0.0
    from sdformerflow_amd import harness
    chunk = harness.prepare_chunk(synth_voxel(2, 10, 144, 144, seed=1234 + 4)).to(DEV)
    label, mask = synth_label(2, 144, 144)
    return model, chunk, label.to(DEV), mask.to(DEV)


def one_step(kind):
    from sdformerflow_amd.spikingjelly_compat import functional
    model, chunk, label, mask = small_model(kind)
    functional.reset_net(model)
    flows = train.forward_train(model, chunk)
    loss = train.flow_loss_supervised(flows, label, mask, 1.0, 1.0)
    loss.backward()
    return model, [f.detach() for f in flows], loss.detach(), {n: p.grad for n, p in model.named_parameters()}


def test_neutral_k_plif_model_equals_the_lif_model():
    """w = 0 everywhere: k = 0.5 exactly, the LIF tau = 2 arithmetic.  One train-mode forward + loss + backward of the PLIF model
    equals the LIF model's within the LIF path's own run-to-run difference (two LIF runs; bit for bit where that is zero).  The
    library's convolution gradients are not bit-reproducible: the PLIF run is a third draw of that noise, so a gradient whose two
    LIF runs differ may sit up to twice their difference plus 1e-6 of its largest element away; one whose LIF runs agree must agree
    bit for bit.  Every node's w.grad is finite and some are non-zero."""
    _, f1, l1, g1 = one_step("lif")
    _, f2, l2, g2 = one_step("lif")
    model, fp, lp, gp = one_step("plif")

    def diff(a, b):
        return (a.float() - b.float()).abs().max().item()

    noise_f = [diff(a, b) for a, b in zip(f1, f2)]
    for a, b, n in zip(fp, f1, noise_f):
        assert diff(a, b) <= n, (diff(a, b), n)
    assert abs(lp.item() - l1.item()) <= abs(l1.item() - l2.item())
    shared = 0
    for name, g in g1.items():
        n = diff(g, g2[name]) if g is not None else 0.0
        assert (gp[name] is None) == (g is None), name
        if g is not None:
            bound = 0.0 if n == 0.0 else 2 * n + 1e-6 * g.abs().max().item()
            assert diff(gp[name], g) <= bound, (name, diff(gp[name], g), n)
            shared += 1
    ws = [m.w.grad for m in model.modules() if isinstance(m, ParametricLIFNode) and m.w.grad is not None]
    assert shared > 100 and len(ws) > 50
    assert all(torch.isfinite(w).all() for w in ws) and any(w.item() != 0.0 for w in ws)


@pytest.mark.parametrize("amp", [False, True])
def test_plif_train_step_moves_every_w(amp):
    model, chunk, label, mask = small_model("plif", w=0.2)
    nodes = [m for m in model.modules() if isinstance(m, ParametricLIFNode)]
    before = [m.w.detach().clone() for m in nodes]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    loss = train.train_step(model, opt, chunk, label, mask, buckets=train.GradientBuckets(model.parameters()), amp=amp)
    assert torch.isfinite(loss).all()
    used = [(m, b) for m, b in zip(nodes, before) if m.w.grad is not None]
    assert len(used) > 50
    assert all(not torch.equal(m.w.detach(), b) for m, b in used)


def test_plif_eval_after_training_uses_the_trained_weights_not_a_stale_engine():
    model, chunk, label, mask = small_model("plif", w=0.2)
    model.eval()
    with torch.no_grad():
        before = [f.clone() for f in model(chunk)["flow"]]
    e0 = model.engine()
    buckets = train.GradientBuckets(model.parameters())
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    for _ in range(2):
        train.train_step(model, opt, chunk, label, mask, buckets=buckets)
    model.eval()
    with torch.no_grad():
        after = [f.clone() for f in model(chunk)["flow"]]
    assert model.engine() is not e0
    assert not any(torch.equal(a, b) for a, b in zip(before, after))
    fresh = MS_SpikingformerFlowNet(*small_kwargs(yaml.safe_load(open(CFG)), "plif"))
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh(chunk)["flow"]
    assert all(torch.equal(a, b) for a, b in zip(after, want))
    # a w moved in place (what optimizer.step() does) is seen through the version stamp
    gate = next(m for m in model.modules() if isinstance(m, ParametricLIFNode))
    e1 = model.engine()
    with torch.no_grad():
        gate.w.add_(0.5)
    assert model.engine() is not e1


def test_plif_function_and_gate_run_without_host_sync():
    x = rnd((10, 4096), 5, -0.3, 0.6).to(DEV).requires_grad_(True)
    g = rnd((10, 4096), 6, -1.0, 2.0).to(DEV)
    w = torch.tensor(0.35, device=DEV, requires_grad=True)
    q = (torch.rand((2, 162, 96), device=DEV) < 0.35).float().requires_grad_(True)
    kk = (torch.rand((2, 162, 96), device=DEV) < 0.3).float().requires_grad_(True)
    ge = torch.randn((2, 162, 96), device=DEV)
    hip.lib()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):                             # the switch does report syncs on this build
            w.detach().sum().item()
        PLIFFunction.apply(x, torch.sigmoid(w), 0.1, None, True, 2.0).backward(g)
        QKGatePLIFFunction.apply(q, kk, torch.sigmoid(w), 5.0, None, True, 2.0).backward(ge)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(w.grad).all() and x.grad is not None and q.grad is not None
