"""Training of the ANN STTFlowNet on the GPU (train_flow_parallel_supervised.py with configs/train_DSEC_supervised_STT_voxel.yml):
one train-mode forward + backward against the reference's own (tests/golden/ann_train_step.npz, make_golden_ann_train.py), one
`train_step` + AdamW at BASELINE configs[2]'s shape, the eval caches after an optimiser step, and seeded stochastic depth."""
import os

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import train
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = ("relative_position_index", "relative_coords_table", "num_batches_tracked")


def build(size, drop_path=True):
    from sdformerflow_amd.STSwinNet import STSwinNet
    from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import SwinTransformerBlock3D
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")))
    net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), dict(cfg["swin_transformer"], input_size=list(size)))
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(SKIP)}), strict=False)
    if not drop_path:                                          # the fixture replaces DropPath by the identity
        for m in net.modules():
            if isinstance(m, SwinTransformerBlock3D):
                m.drop_path = 0.0
    return net.cuda()


def test_train_step_matches_the_reference_fixture():
    G = np.load(os.path.join(ROOT, "tests", "golden", "ann_train_step.npz"))
    B, BINS, H, W, SEED = (int(v) for v in G["cfg"])
    net = build((H, W), drop_path=False).train()
    vox = synth_voxel(B, BINS, H, W, seed=SEED).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=SEED + 1))
    flows = net(vox, None)["flow"]
    loss = train.flow_loss_supervised(flows, label, mask, float(G["flow_scaling"]), float(G["lambda_mod"]))
    loss.backward()
    assert abs(loss.item() - float(G["loss"])) <= 1e-5 * abs(float(G["loss"])), (loss.item(), float(G["loss"]))      # measured 1.5e-7
    for i, f in enumerate(flows):
        ref = float(G[f"flow{i}_abs_mean"])
        assert abs(f.abs().mean().item() - ref) <= 1e-5 * ref, (i, f.abs().mean().item(), ref)
    params = dict(net.named_parameters())
    names = [str(n) for n in G["grad_names"]]
    assert names == list(params), "parameter names differ from the reference's"
    assert all(p.grad is not None for p in params.values()), [n for n, p in params.items() if p.grad is None]
    worst = 0.0
    for n, r in zip(names, G["grad_norms"]):
        got = params[n].grad.double().norm().item()
        worst = max(worst, abs(got - r) / r)
        assert abs(got - r) <= 1e-3 * r, (n, got, r)
    for k in G.files:
        if k.startswith("g/"):
            ref = torch.from_numpy(G[k]).double()
            d = (params[k[2:]].grad.cpu().double() - ref).abs().max().item()
            assert d <= 1e-3 * ref.abs().max().item(), (k, d, ref.abs().max().item())
        elif k.startswith("r/"):
            buf = dict(net.named_buffers())[k[2:]].cpu().double()
            ref = torch.from_numpy(G[k]).double()
            assert (buf - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), k
    print(f"ann train step vs reference: loss {loss.item():.8f} / {float(G['loss']):.8f}, worst gradient-norm deviation {worst:.2e}, "
          "flow abs-mean deviations " + ", ".join(f"{abs(f.abs().mean().item() / float(G[f'flow{i}_abs_mean']) - 1):.1e}" for i, f in enumerate(flows)))


def test_config2_train_step_then_eval():
    """BASELINE configs[2]'s shape (B = 8, 288 x 384): one train_step + AdamW (clip_grad None, as the STT_voxel config) gives a finite
    loss; the eval flows afterwards are finite, differ from the pre-step flows, and equal those of a fresh model holding the
    stepped weights - every packed-weight cache of the eval path was rebuilt after the optimiser's in-place updates."""
    torch.manual_seed(11)
    B, H, W = 8, 288, 384
    net = build((H, W))
    vox = synth_voxel(B, 20, H, W, seed=808).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=809))
    net.eval()
    before = [f.clone() for f in net(vox, None)["flow"]]           # fills every eval cache with the pre-step weights
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.01)
    loss = train.train_step(net, opt, vox, label, mask, clip_grad=None)
    assert torch.isfinite(loss).item()
    assert all(p.grad is not None for p in net.parameters())
    net.eval()
    after = net(vox, None)["flow"]
    fresh = build((H, W))
    fresh.load_state_dict(net.state_dict())
    ref = fresh.eval()(vox, None)["flow"]
    for a, b0, r in zip(after, before, ref):
        assert torch.isfinite(a).all()
        assert (a - b0).abs().max().item() > 1e-3 * b0.abs().max().item()
        assert (a - r).abs().max().item() <= 1e-5 * r.abs().max().item()


def test_drop_path_is_reproducible_under_a_seed():
    B, H, W = 2, 144, 192
    net = build((H, W)).train()
    vox = synth_voxel(B, 20, H, W, seed=5).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=6))

    def run(seed):
        net.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        loss = train.flow_loss_supervised(net(vox, None)["flow"], label, mask)
        loss.backward()
        return loss.item(), [p.grad.clone() for p in net.parameters()]
    l1, g1 = run(7)
    l2, g2 = run(7)
    l3, _ = run(8)
    assert l1 == l2
    # (the library's gather backward of the position-bias table accumulates with atomics: gradients agree to rounding, not bits)
    assert all((a - b).abs().max().item() <= 1e-5 * b.abs().max().item() for a, b in zip(g1, g2))
    assert l3 != l1                                            # the stochastic depth is live: another seed, other samples dropped
