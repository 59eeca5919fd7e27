"""Fine-tuning at a window above 192 tokens: STTFlowNet (ANN) and SpikingformerFlowNet (SEW) at window (2,15,15) - 450 tokens - with the
HIP attention both ways (csrc/win_attn_large.hip forward, csrc/win_attn_large_bwd.hip backward), which SDF_ANN_ATTN_BWD=2 /
SDF_SEW_ATTN_BWD=2 opt in to.  The models are the 240 x 240 three-stage ones of tests/test_large_window_models_gpu.py (builders
restated here).  With the switch unset the refusal that file pins still stands; at 2 a window above 1024 tokens is refused before any
launch."""
import copy
import os
import re

import pytest
import torch
import yaml

import win_attn_large_bwd_cases as LC
from routes_common import short
from sdformerflow_amd import harness, hip, train
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_uniform as rnd, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_ANN = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")
CFG_SNN = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
WS, SS, PWS, SIZE = (2, 15, 15), (1, 7, 7), (2, 9, 9), (240, 240)
DERIVED = ("relative_position_index", "relative_coords_table", "num_batches_tracked")
FWD = "win_attn_large_kernel"
ANN_BWD = ["win_attn_large_ann_bwd_query_kernel", "win_attn_large_ann_bwd_key_kernel", "win_attn_large_ann_bwd_dbias_kernel",
           "win_attn_large_bwd_sum_runs_kernel", "win_attn_large_ann_bwd_reduce_kernel"]
SEW_BWD = ["win_attn_large_sew_bwd_gram_kernel", "win_attn_large_sew_bwd_dv_kernel", "win_attn_large_sew_dbias_kernel", "win_attn_large_bwd_sum_runs_kernel"]
SMALL = ("win_attn_kernel", "win_attn_tiled_kernel", "win_attn_ann_bwd_kernel", "win_attn_ann_bwd_reduce_kernel", "sew_bwd_kernel",
         "sew_bwd_dbias_kernel", "sew_bwd_dbias_finish_kernel")        # the <= 192 entry points' kernels


def _attention_kernels(log):
    """the window-attention launches of a log, by short name -> count; none of the <= 192 kernels among them"""
    names = [re.sub(r"<.*$", "", short(r[0])) for r in log.rows]          # (without template arguments)
    assert not any(n in SMALL for n in names), names
    return {n: names.count(n) for n in names if "win_attn" in n}


# ---------------------------------------------------------------------------------------------------------------- ANN
def _ann_model(window, pws):
    from sdformerflow_amd.STSwinNet import STSwinNet
    cfg = yaml.safe_load(open(CFG_ANN))
    swin = dict(cfg["swin_transformer"], input_size=list(SIZE), window_size=list(window), pretrained_window_size=list(pws))
    net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), swin)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(DERIVED)})
    net.load_state_dict(sd, strict=False)
    net.norm_input = False
    return net


def _ann_step(net, value):
    """one train_step of a copy of `net` under SDF_ANN_ATTN_BWD=value -> (loss, {name: gradient}, launch log)"""
    net = copy.deepcopy(net).to(DEV)
    vox = synth_voxel(1, 20, *SIZE, seed=2237).to(DEV)
    label, mask = (t.to(DEV) for t in synth_label(1, *SIZE, seed=2238))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.01)
    torch.manual_seed(5)                                       # the DropPath draws of the step
    with hip.scoped_switches(SDF_ANN_ATTN_BWD=value), hip.launch_log() as log:
        loss = train.train_step(net, opt, vox, label, mask, clip_grad=None)
    torch.cuda.synchronize()
    return loss.item(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}, log


def test_ann_train_step_on_the_hip_backward_equals_the_torch_composition(monkeypatch):
    """One train_step under SDF_ANN_ATTN_BWD=2 and one under 0, from the same weights and the same seed (identical DropPath draws): the
    losses agree to 1e-5 relative and every parameter gradient is within 1e-3 of its largest element (the bound of
    tests/test_ann_train_gpu.py).  Measured on an MI355X: the two losses are the same fp32 number (6.46023321), the worst gradient is
    4.0e-06 of its largest element (3.8e-06 in a second run; a cpb_mlp weight or logit_scale of the last stage).  Under 2 the log holds the large forward and the five backward
    kernels once per block (ten blocks), none of the <= 192 kernels, and the torch composition (the only softmax of the model) is never
    called."""
    from sdformerflow_amd.STSwinNet import swin_transformer3D_v2 as sw
    net = _ann_model(WS, PWS)
    loss0, grads0, log0 = _ann_step(net, "0")
    assert not any("win_attn" in r[0] for r in log0.rows)

    def never(*a, **k):
        raise AssertionError("the torch composition of the attention was called under SDF_ANN_ATTN_BWD=2")
    monkeypatch.setattr(sw, "attention_rows_torch", never)
    loss2, grads2, log2 = _ann_step(net, "2")
    assert _attention_kernels(log2) == dict({FWD: 10}, **{n: 10 for n in ANN_BWD})
    print(f"ann window 15 train step: loss {loss2:.8e} (HIP) {loss0:.8e} (torch), relative difference {abs(loss2 - loss0) / abs(loss0):.2e}")
    assert abs(loss2 - loss0) <= 1e-5 * abs(loss0), (loss2, loss0)
    worst = ("", 0.0)
    for n, g0 in grads0.items():
        assert torch.isfinite(grads2[n]).all(), n
        rel = (grads2[n] - g0).abs().max().item() / max(g0.abs().max().item(), 1e-30)
        worst = max(worst, (n, rel), key=lambda t: t[1])
    print(f"    worst gradient: {worst[1]:.2e} of its largest element ({worst[0]})")
    assert worst[1] <= 1e-3, worst
    assert any(float(g.abs().max()) > 0 for n, g in grads2.items() if "cpb_mlp" in n)


def test_ann_refusals_at_the_default_and_above_1024_tokens():
    from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import WindowAttention3D
    net = _ann_model(WS, PWS).to(DEV).train()
    vox = synth_voxel(1, 20, *SIZE, seed=2237).to(DEV)
    with hip.launch_log() as log, pytest.raises(NotImplementedError, match="SDF_ANN_ATTN_BWD=0") as e:
        net(vox, None)
    assert not log.rows and "192" in str(e.value) and "SDF_ANN_ATTN_BWD=2" in str(e.value)
    attn = WindowAttention3D(96, (2, 23, 23), (0, 0, 0), 3, qkv_bias=True).to(DEV).train()            # 1058 tokens
    with hip.scoped_switches(SDF_ANN_ATTN_BWD="2"), hip.launch_log() as log, pytest.raises(NotImplementedError, match="1024"):
        attn.forward_train_rows(torch.zeros(1058, 96, device=DEV), torch.arange(1058, dtype=torch.int32, device=DEV), 1, None)
    assert not log.rows, log.rows


# ---------------------------------------------------------------------------------------------------------------- SEW
def _kw(kind, T):
    return {"num_steps": T, "v_reset": None, "v_th": 0.1, "neuron_type": kind, "surrogate_fun": "surrogate.ATan()", "tau": 2.0,
            "detach_reset": True, "spike_norm": "BN"}


def _sew_model(window):
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    cfg = yaml.safe_load(open(CFG_SNN))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"].update(input_size=list(SIZE), window_size=list(window), swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12],
                                   swin_out_indices=[0, 1, 2])
    model = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(("relative_position_index",))})
    model.load_state_dict(sd, strict=False)
    return model


def _sew_attention_module():
    from sdformerflow_amd.STSwinNet_SNN import Spiking_swin_transformer3D as SW
    blk = SW.Spiking_SwinTransformerBlock3D(96, (30, 45), 3, window_size=WS, shift_size=SS, qk_scale=0.125, norm_layer="BN", **_kw("lif", 4))
    sd = synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items() if not k.endswith(("relative_position_index",))})
    blk.load_state_dict(sd, strict=False)
    return blk.attn.to(DEV).train()


def test_sew_attention_module_on_the_hip_backward_equals_the_torch_composition():
    """`train.sew_attention` on one attention module, input (2, 1, 225, 96) (one 450-token window, masked), under SDF_SEW_ATTN_BWD=2 and
    under 0: the same q | k | v spikes on both routes, and the output and every gradient (input, Linear, BN, bias table) within 1e-4 of
    the tensor's largest element.  One tensor has no largest element to measure against: proj.bias stands in front of a
    batch-statistics BN, its true gradient is 0 and both routes hold rounding noise there (tests/test_sew_train_gpu.py treats it the same
    way), so its values on both routes and their difference are held to 1e-4 of the largest element of proj.weight's gradient instead.
    Measured on an MI355X: the outputs are equal, the worst gradient is 1.11e-06 of its largest
    element (linear_v.weight); proj.bias 1.7e-07 in absolute terms, 2.3e-09 of the largest element of proj.weight's gradient."""
    from sdformerflow_amd.spikingjelly_compat import functional
    attn = _sew_attention_module()
    x0 = ((rnd((2, 1, 225, 96), 41) > 0.5).float() + (rnd((2, 1, 225, 96), 42) > 0.7).float()).to(DEV)      # a sum of spike tensors
    w = rnd((2, 1, 225, 96), 43, -1.0, 1.0).to(DEV)
    mask = LC.label_mask(1, 450, torch.Generator().manual_seed(44)).to(DEV).contiguous()
    runs = {}
    for value in ("2", "0"):
        functional.reset_net(attn)
        attn.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        tape = {}
        hooks = [getattr(attn, "sn_" + n).register_forward_hook(lambda m, i, o, n=n: tape.__setitem__(n, o.detach().clone())) for n in "qkv"]
        with hip.scoped_switches(SDF_SEW_ATTN_BWD=value), hip.launch_log() as log:
            out = train.sew_attention(x, attn, mask)
            (out * w).sum().backward()
        for h in hooks:
            h.remove()
        torch.cuda.synchronize()
        grads = {"input": x.grad.detach().clone()}
        grads.update({n: p.grad.detach().clone() for n, p in attn.named_parameters() if p.grad is not None})
        runs[value] = (out.detach().clone(), grads, tape, log)
    out2, g2, tape2, log2 = runs["2"]
    out0, g0, tape0, log0 = runs["0"]
    assert _attention_kernels(log2) == dict({FWD: 1}, **{n: 1 for n in SEW_BWD})
    assert not any("win_attn" in r[0] for r in log0.rows)
    assert all(torch.equal(tape2[n], tape0[n]) and tape2[n].any() for n in "qkv")
    assert set(g2) == set(g0) and "relative_position_bias_table" in g2 and any(n.startswith("linear_q") for n in g2)
    assert any(n.startswith("bn_q") for n in g2)
    report = {"output": (out2 - out0).abs().max().item() / out0.abs().max().item()}
    for n in g0:
        report[n] = (g2[n] - g0[n]).abs().max().item() / max(g0[n].abs().max().item(), 1e-30)
    worst = max(report, key=report.get)
    print(f"sew attention window 15, HIP vs torch composition: output {report['output']:.2e}, worst gradient {report[worst]:.2e} ({worst})")
    wtop = g0["proj.weight"].abs().max().item()
    noise = max(g2["proj.bias"].abs().max().item(), g0["proj.bias"].abs().max().item(), (g2["proj.bias"] - g0["proj.bias"]).abs().max().item())
    print(f"    proj.bias (true gradient 0): largest |value| or difference {noise:.2e} = {noise / wtop:.2e} of max |d proj.weight| {wtop:.2e}")
    for n, r in report.items():
        if n == "proj.bias":
            assert noise <= 1e-4 * wtop, (n, noise, wtop)
        else:
            assert r <= 1e-4, (n, r)
    assert float(g2["relative_position_bias_table"].abs().max()) > 0


def test_sew_model_trains_at_window_15_on_the_hip_kernels():
    """Under SDF_SEW_ATTN_BWD=2 one forward_train_sew + loss + backward (train.train_step) completes: the large kernels both ways once per
    block, every gradient finite, the relative-position tables trained.  (No cross-route comparison at model level: the forward's
    rounding differs between the routes and spikes downstream may flip.)"""
    model = _sew_model(WS).to(DEV)
    chunk = harness.prepare_chunk(synth_voxel(1, 10, *SIZE, seed=3241)).to(DEV)
    label, mask = (t.to(DEV) for t in synth_label(1, *SIZE, seed=3242))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    torch.manual_seed(7)
    with hip.scoped_switches(SDF_SEW_ATTN_BWD="2"), hip.launch_log() as log:
        loss = train.train_step(model, opt, chunk, label, mask, clip_grad=None)
    torch.cuda.synchronize()
    assert _attention_kernels(log) == dict({FWD: 10}, **{n: 10 for n in SEW_BWD})
    assert torch.isfinite(loss).all()
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()), [n for n, g in grads.items() if g is None]
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    tables = [g for n, g in grads.items() if n.endswith("relative_position_bias_table")]
    assert len(tables) == 10 and all(float(g.abs().max()) > 0 for g in tables)


def test_sew_refusals_at_the_default_and_above_1024_tokens():
    model = _sew_model(WS).to(DEV).train()
    chunk = harness.prepare_chunk(synth_voxel(1, 10, *SIZE, seed=3241)).to(DEV)
    with hip.launch_log() as log, pytest.raises(NotImplementedError, match="SDF_SEW_ATTN_BWD=0") as e:
        train.forward_train_sew(model, chunk)
    assert not log.rows and "192" in str(e.value) and "SDF_SEW_ATTN_BWD=2" in str(e.value)
    attn = model.sttmultires_unet.encoders.swin3d.layers[0].swin_blocks[0].attn
    with hip.scoped_switches(SDF_SEW_ATTN_BWD="2"), hip.launch_log() as log, pytest.raises(NotImplementedError, match="1024"):
        train.sew_attention(torch.zeros(2, 1, 529, 96, device=DEV), attn, None)                           # 1058 tokens
    assert not log.rows, log.rows
