"""Training of the SEW family (SpikingformerFlowNet) on the GPU: the train-mode SEW block against the real reference's autograd
(tests/golden/sew_train_block.npz), the whole-model step against the CPU oracle with the GPU's spikes forced (the oracle is pinned on
the reference the same way: tests/golden/sew_train_step_forced.npz), with the HIP attention backward and with SDF_SEW_ATTN_BWD=0,
AdamW steps, bf16 autocast, and eval after training."""
import os

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import hip, train
from sdformerflow_amd.STSwinNet_SNN import Spiking_swin_transformer3D as SW
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_uniform as rnd, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
TB = np.load(os.path.join(HERE, "golden", "sew_train_block.npz"))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
SKIP = ("relative_position_index", "num_batches_tracked")


def kw(kind, T):
    return {"num_steps": T, "v_reset": None, "v_th": 0.1, "neuron_type": kind, "surrogate_fun": "surrogate.ATan()", "tau": 2.0,
            "detach_reset": True, "spike_norm": "BN"}


def load_synth(mod):
    mod.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in mod.state_dict().items() if not k.endswith(SKIP)}), strict=False)
    for m in mod.modules():
        if hasattr(m, "drop_path_rate"):
            m.drop_path_rate = 0.0                                     # the fixtures were made with DropPath = identity
    return mod.to(DEV).train()


def rate(got, ref):
    got, ref = got.detach().float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape
    scale = ref.abs().mean().item() + 1e-12
    return ((got - ref).abs() > 1e-3 * scale).float().mean().item()


def picked(t, key):
    """The elements of t the fixture kept under `key` (all of them, or those at `key@idx`), flattened."""
    t = t.detach().reshape(-1)
    return t[torch.from_numpy(TB[key + "@idx"]).long().to(t.device)] if key + "@idx" in TB.files else t


@pytest.mark.parametrize("tag", ["lif_w", "lif_sw", "psn_w", "psn_sw"])
def test_train_mode_sew_block_matches_reference_autograd(tag):
    """Mismatch rates over the elements the fixture kept, with the bounds of the MS block (tests/test_train_gpu.py)."""
    B, D, H, W, *shift = (int(v) for v in TB[f"{tag}_cfg"])
    kind = tag.split("_")[0]
    blk = load_synth(SW.Spiking_SwinTransformerBlock3D(96, (H, W), 3, window_size=(2, 9, 9), shift_size=tuple(shift), norm_layer="BN",
                                                       qk_scale=0.125, **kw(kind, D)))
    assert blk.attn.scale == float(TB[f"{tag}_scale"])
    x = rnd((B, D, H, W, 96), 21, -0.5, 1.5).to(DEV).requires_grad_(True)
    g = rnd((B, D, H, W, 96), 22, -1.0, 2.0).to(DEV)
    y = train.sew_block(x, blk, training=True)
    y.backward(g)
    report = {"y": rate(picked(y, f"{tag}_y"), TB[f"{tag}_y"]), "gx": rate(picked(x.grad, f"{tag}_gx"), TB[f"{tag}_gx"])}
    params, bufs = dict(blk.named_parameters()), dict(blk.named_buffers())
    seen = set()
    for k in TB.files:
        if k.endswith("@idx"):
            continue
        if k.startswith(tag + "_g/"):
            name = k[len(tag) + 3:]
            seen.add(name)
            if name.endswith("proj.bias"):                 # a bias in front of a batch-stat BN: rounding noise on both sides
                assert params[name].grad.abs().max().item() < 1e-3 * float(np.abs(TB[f"{tag}_g/attn.proj.weight"]).mean())
            else:
                report[name] = rate(picked(params[name].grad, k), TB[k])
        elif k.startswith(tag + "_r/"):
            name = k[len(tag) + 3:]
            report["running:" + name] = rate(picked(bufs[name], k), TB[k])
    assert "attn.relative_position_bias_table" in seen
    worst = max(report.values())
    print(f"sew train block {tag}: mismatch rates y {report['y']:.2e} gx {report['gx']:.2e} worst {worst:.2e} "
          f"({max(report, key=report.get)})")
    assert report["y"] <= 2e-3 and report["gx"] <= 5e-3 and worst <= 1e-2, report


def small_model(kind="lif"):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"].update(input_size=[144, 192], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    model = load_synth(SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy()))
    from sdformerflow_amd import harness
    chunk = harness.prepare_chunk(synth_voxel(2, 10, 144, 192, seed=1234 + 9)).to(DEV)
    label, mask = synth_label(2, 144, 192)
    return model, chunk, label.to(DEV), mask.to(DEV), cfg


@pytest.mark.parametrize("kind,attn", [("lif", "hip"), ("psn", "hip"), ("lif", "torch")])
def test_sew_train_step_spike_forced_gradient_parity(kind, attn):
    """One train-mode forward + loss + backward of the 3-encoder SEW model (144 x 192, batch 2) with every neuron's spikes kept; the
    CPU oracle then runs its TRAIN-mode `forward_sew_flownet` with those spikes forced.  0 unexplained decisions, loss to 1e-6, every
    parameter gradient within 2e-4 of its largest element - with the HIP attention backward and with its torch composition
    (SDF_SEW_ATTN_BWD=0), so the two paths agree within that bound too."""
    from oracle import sdformer_oracle as O
    model, chunk, label, mask, _ = small_model(kind)
    tape = {}
    hooks = [m.register_forward_hook(lambda mod, inp, o, n=n: tape.__setitem__(n + ".", o.detach().to(torch.uint8).cpu()))
             for n, m in model.named_modules() if n.endswith(".spiking_neuron")]
    with hip.scoped_switches(SDF_SEW_ATTN_BWD="0" if attn == "torch" else None):
        loss = train.flow_loss_supervised(model(chunk)["flow"], label, mask, 1.0, 1.0)
        loss.backward()
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(SKIP)}
    sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and not k.endswith(("running_mean", "running_var")) else v.clone())
          for k, v in synth_state_dict(shapes).items()}                     # the weights BEFORE the step (running statistics moved)
    ncfg = O.NeuronCfg(kind, 0.1, None, 2.0, 10)
    ocfg = {"neuron": ncfg, "num_bins": 10, "window_size": (2, 9, 9), "depths": [2, 2, 6], "num_heads": [3, 6, 12]}
    report = []

    def force(prefix, x):
        got = tape[prefix]
        xd = x.detach()
        delta = 16 * 2.0 ** -23 * max(float(xd.pow(2).mean().sqrt()), 0.1)
        r = O.delta_consistent(xd, got.reshape(xd.shape).float(), ncfg, {k: v.detach() for k, v in sd.items()}, prefix, delta)
        report.append((prefix, r["flips"], r["unexplained"], r["n"]))
        return got.reshape(x.shape).float()

    O.TRAIN, O.NEURON_FORCE = O.TrainCtx(), force
    try:
        with torch.enable_grad():
            oloss = O.flow_loss_supervised(O.forward_sew_flownet(chunk.cpu(), sd, ocfg), label.cpu(), mask.cpu(), 1.0, 1.0)
            oloss.backward()
    finally:
        O.TRAIN, O.NEURON_FORCE = None, None
    flips, unexplained, n = (sum(r[i] for r in report) for i in (1, 2, 3))
    assert len(report) == len(tape) == 75 and unexplained == 0, [r for r in report if r[2]][:5]
    assert flips <= 2e-6 * n, (flips, n)
    assert abs(loss.item() - oloss.item()) <= 1e-6 * abs(oloss.item()), (loss.item(), oloss.item())
    worst, worst_name, checked = 0.0, "", 0
    for name, p in model.named_parameters():
        og = sd[name].grad
        if og is None or float(og.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        scale = sd[name[:-4] + "weight"].grad.abs().max() if name.endswith("attn.proj.bias") else og.abs().max()
        dev = float((p.grad.cpu() - og).abs().max() / scale)
        checked += 1
        if dev > worst:
            worst, worst_name = dev, name
    print(f"sew train step, spikes forced ({kind}, attention {attn}): {n} decisions, {flips} differ, 0 unexplained; loss {loss.item():.8f} "
          f"vs {oloss.item():.8f}; {checked} gradients, worst {worst:.2e} ({worst_name})")
    assert checked >= 150 and worst <= 2e-4, (worst, worst_name)


def test_adamw_steps_amp_and_eval_after_training():
    """train_step (reset, forward, loss, backward, clip 100, AdamW) on a fixed micro-batch: the loss goes down and the running
    statistics move; a bf16-autocast step gives a finite loss; eval afterwards serves the trained weights (equal to a fresh model
    holding the same state_dict), not the engine packed before training."""
    model, chunk, label, mask, cfg = small_model("lif")
    model.eval()
    with torch.no_grad():
        before = [f.clone() for f in model(chunk)["flow"]]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    rm = model.sttmultires_unet.encoders.swin3d.layers[0].swin_blocks[1].attn.bn_q.norm_layer.running_mean
    rm0 = rm.clone()
    buckets = train.GradientBuckets(model.parameters())
    losses = [train.train_step(model, opt, chunk, label, mask, buckets=buckets).item() for _ in range(6)]
    print("sew losses", ["%.4f" % v for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert not torch.equal(rm0, rm)
    assert model.sttmultires_unet.encoders.swin3d.layers[0].swin_blocks[1].attn.relative_position_bias_table.grad.abs().max() > 0
    amp_loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, amp=True)
    assert torch.isfinite(amp_loss).item()
    model.eval()
    with torch.no_grad():
        after = [f.clone() for f in model(chunk)["flow"]]
    assert not any(torch.equal(a, b) for a, b in zip(before, after))
    fresh = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    fresh.load_state_dict(model.state_dict(), strict=True)
    with torch.no_grad():
        want = fresh.to(DEV).eval()(chunk)["flow"]
    assert all(torch.equal(a, b) for a, b in zip(after, want))
