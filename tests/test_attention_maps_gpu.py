"""`log=True` and `return_attention=True` of the ANN (STTFlowNet) and SEW (SpikingformerFlowNet) families: the attention map
(B_, nH, N, N) of the last block of every stage, made by csrc/win_attn_scores.hip during the one forward that makes the flows.

Models: the smallest the end-to-end tests build - the STTFlowNet of ann_end_to_end.npz (tests/test_ann_model.py, 144 x 192, batch 2),
the SpikingformerFlowNet of sew_end_to_end.npz (144 x 192, lif and psn), and the 240 x 240 window-(2,15,15) ANN model of
tests/test_large_window_models_gpu.py (450 tokens per window).

ANN.  Flows bit-equal to the log=False flows; one map per stage of shape (B * nW_s, nH_s, N, N); each bit-equal to
hip.win_attn_ann_scores called here on the last block's input (forward pre-hook) through the package's own layer_norm and linear_rows
with the block's row map, mask, bias and scale; each within 1e-3 of the fp64 composition from the same hooked input (O.slice_table +
O.ann_attention_core).  That is a plumbing bound: a wrong block, shift, mask or stage order is an O(1) error, while the fp16-plane
qkv product's 2^-22 error moves a probability by under 1e-4 at logit scale 10; the value bound is tests/test_win_attn_scores_gpu.py's.
(The ANN U-Net's plain convolutions run in the library, whose default solver choice does not reproduce its own bits from one call to
the next at this size: two log=False forwards differ by 1.7e-6 in every flow, while the encoder's features are bit-equal.  The flow
comparison therefore runs both forwards under torch.backends.cudnn.deterministic, where plain forwards repeat bit for bit.)
SEW.  Flows bit-equal with and without log; with the parity tape on in the same forward each stage's map meets that file's SEW bound,
|a - a64| <= 2^-22 (c scale + |bias| + |mask|), against O.sew_attention_core in fp64 on the taped attn.sn_q / attn.sn_k spikes of the
stage's last block with that block's bias, scale and mask.

Measured on an MI355X: SEW max |a - a64| / S 6.0e-8 at every stage, lif and psn (bound 2.4e-7), block level the same; ANN max |p - p64| 3.3e-7 / 2.1e-7 / 2.6e-7 at the three stages (bound 1e-3).
Run time there: the 8 cases of this file in 7 s together (3.8 s of it the batch-2 ANN model with its fp64 compositions)."""
import contextlib
import functools
import os

import pytest
import torch
import yaml

from oracle import sdformer_oracle as O
from sdformerflow_amd import harness, hip, module_forward
from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import layer_norm, linear_rows
from sdformerflow_amd.STSwinNet_SNN.Spiking_swin_transformer3D import get_window_size
from sdformerflow_amd.synthetic import synth_state_dict, synth_uniform as rnd, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_ANN = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")
CFG_SNN = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
DERIVED = ("relative_position_index", "relative_coords_table", "num_batches_tracked")
PLUMBING_TOL = 1e-3
SEW_REL = 2.0 ** -22
KERNEL = "win_attn_scores_kernel"


# ---------------------------------------------------------------------------------------------------------------- ANN
@functools.lru_cache(maxsize=None)
def _ann_model(size, window, pws):
    from sdformerflow_amd.STSwinNet import STSwinNet
    cfg = yaml.safe_load(open(CFG_ANN))
    swin = dict(cfg["swin_transformer"], input_size=list(size), window_size=list(window), pretrained_window_size=list(pws))
    net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), swin)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(DERIVED)})
    net.load_state_dict(sd, strict=False)
    net.norm_input = False
    return net.to(DEV).eval()


@contextlib.contextmanager
def _deterministic_library_convolutions():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


def _pad3(D, H, W, ws):
    return D + (-D) % ws[0], H + (-H) % ws[1], W + (-W) % ws[2]


def _ann_direct(blk, x_in, want64=True):
    """(the map by a direct hip.win_attn_ann_scores call, the fp64 composition or None) from the block's hooked input (B,D,H,W,C)."""
    B, D, H, W, C = x_in.shape
    ws, ss = get_window_size((D, H, W), blk.window_size, blk.shift_size)
    N, nH = ws[0] * ws[1] * ws[2], blk.num_heads
    with torch.no_grad():
        qkv = linear_rows(blk.attn.qkv, layer_norm(blk.norm1, x_in).reshape(-1, C))
        bias, scale = blk.attn._bias_and_scale()
        pad = blk.attn.qkv.bias.detach().float().contiguous()
    mask = O.compute_mask(*_pad3(D, H, W, ws), ws, ss) if any(s > 0 for s in ss) else None
    row_map, B_ = hip.window_slice_map(B, D, H, W, ws, ss, DEV)
    with hip.launch_log() as log:
        got = hip.win_attn_ann_scores(qkv, scale, bias, None if mask is None else mask.to(DEV), nH, row_map, B_, N, pad)
    assert len(log.rows) == 1 and KERNEL in log.rows[0][0]
    if not want64:
        return got, None
    src, B2 = O.slice_table(B, D, H, W, ws, ss)
    assert B2 == B_
    src = torch.from_numpy(src).reshape(B_, N)
    flat = torch.cat([qkv.cpu().double(), pad.cpu().double()[None]], 0)
    win = flat[torch.where(src < 0, torch.tensor(flat.shape[0] - 1), src)]
    _, p64 = O.ann_attention_core(win, scale.cpu().double().view(nH, 1, 1), bias.cpu().double(), None if mask is None else mask.double(), nH)
    return got, p64


def _ann_log_forward(net, vox):
    """-> (log=False flows, log=True output, hooked inputs of the last block of every stage, launch rows of the log=True forward)."""
    layers = net.sttmultires_unet.encoders.swin3d.layers
    seen = [[] for _ in layers]
    hooks = [layer.swin_blocks[-1].register_forward_pre_hook(lambda m, args, s=s: seen[s].append(args[0])) for s, layer in enumerate(layers)]
    try:
        with _deterministic_library_convolutions():
            plain = net(vox, None)["flow"]
            for s in seen:
                s.clear()
            with hip.launch_log() as log:
                out = net(vox, None, log=True)
    finally:
        for h in hooks:
            h.remove()
    assert all(len(s) == 2 and s[0] is s[1] for s in seen)        # the map and the block's own forward take the same input
    return plain, out, [s[0] for s in seen], log


def _check_ann_maps(net, vox, what, value_check=True):
    layers = net.sttmultires_unet.encoders.swin3d.layers
    plain, out, inputs, log = _ann_log_forward(net, vox)
    assert len(out["flow"]) == len(plain) and all(torch.equal(a, b) for a, b in zip(out["flow"], plain)), "log=True changed the flows"
    assert sum(KERNEL in r[0] for r in log.rows) == len(layers)
    maps = out["attn"]
    assert isinstance(maps, list) and len(maps) == len(layers)
    for s, (layer, m, x_in) in enumerate(zip(layers, maps, inputs)):
        blk = layer.swin_blocks[-1]
        B, D, H, W, C = x_in.shape
        ws, _ = get_window_size((D, H, W), blk.window_size, blk.shift_size)
        Dp, Hp, Wp = _pad3(D, H, W, ws)
        N, nWin = ws[0] * ws[1] * ws[2], (Dp // ws[0]) * (Hp // ws[1]) * (Wp // ws[2])
        assert m.shape == (B * nWin, blk.num_heads, N, N) and m.dtype == torch.float32 and m.is_cuda, (s, m.shape)
        direct, p64 = _ann_direct(blk, x_in, value_check)
        assert torch.equal(m, direct), f"stage {s}: not the map of the last block's input"
        if value_check:
            err = (m.cpu().double() - p64).abs().max().item()
            print(f"\nATTN_MAPS {what} stage {s}: {tuple(m.shape)} max |p - p64| {err:.3e}")
            assert err <= PLUMBING_TOL, (s, err)
        with torch.no_grad():
            assert torch.equal(blk(x_in, None, return_attention=True), m)
    return maps, inputs


def test_sttflownet_log_true_returns_the_maps_of_one_forward():
    net = _ann_model((144, 192), (2, 9, 9), (0, 0, 0))
    vox = synth_voxel(2, 20, 144, 192, seed=1237).to(DEV)
    maps, inputs = _check_ann_maps(net, vox, "STTFlowNet 144x192")
    enc = net.sttmultires_unet.encoders.swin3d
    x = torch.stack(list(vox.chunk(net.num_split, dim=1)), dim=0)                 # what STTFlowNet.forward hands its U-Net
    with torch.no_grad():
        again = enc.get_layer_attention_scores(x)
        assert len(again) == len(maps) and all(torch.equal(a, b) for a, b in zip(again, maps))
        # the layer-level entry point, from the stage's own input: the hooked input of the last block is what the blocks before it made
        first = []
        h = enc.layers[0].register_forward_pre_hook(lambda m, args: first.append(args[0]))
        try:
            enc(x)
        finally:
            h.remove()
        assert torch.equal(enc.layers[0].get_lst_block_attention_scores(first[0]), maps[0])


def test_sttflownet_log_true_at_window_15():
    """450 tokens per window (the key-blocked range of the forward): shapes, bit-equality with the direct call, unchanged flows."""
    net = _ann_model((240, 240), (2, 15, 15), (2, 9, 9))
    vox = synth_voxel(1, 20, 240, 240, seed=2237).to(DEV)
    maps, _ = _check_ann_maps(net, vox, "STTFlowNet 240x240 window 15", value_check=False)
    assert [tuple(m.shape) for m in maps] == [(16, 3, 450, 450), (4, 6, 450, 450), (1, 12, 450, 450)]


def test_ann_refusals_happen_before_any_launch():
    net = _ann_model((144, 192), (2, 9, 9), (0, 0, 0))
    vox = synth_voxel(1, 20, 144, 192, seed=1238).to(DEV)
    blk = net.sttmultires_unet.encoders.swin3d.layers[0].swin_blocks[-1]
    net.train()
    try:
        with hip.launch_log() as log, pytest.raises(NotImplementedError, match="eval mode"):
            net(vox, None, log=True)
        assert not log.rows, log.rows
        with hip.launch_log() as log, pytest.raises(NotImplementedError, match="eval mode"):
            blk(torch.zeros(1, 2, 36, 48, 96, device=DEV), None, return_attention=True)
        assert not log.rows, log.rows
        with hip.launch_log() as log, pytest.raises(NotImplementedError, match="eval mode"):
            net.sttmultires_unet.encoders.swin3d.get_layer_attention_scores(torch.zeros(2, 1, 10, 144, 192, device=DEV))
        assert not log.rows, log.rows
    finally:
        net.eval()


# ---------------------------------------------------------------------------------------------------------------- SEW
@functools.lru_cache(maxsize=None)
def _sew_model(kind):
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    cfg = yaml.safe_load(open(CFG_SNN))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=10)
    cfg["model"]["num_bins"] = 10
    cfg["swin_transformer"].update(input_size=[144, 192], window_size=[2, 9, 9], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12],
                                   swin_out_indices=[0, 1, 2])
    model = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(("relative_position_index",))})
    model.load_state_dict(sd, strict=False)
    return model.eval().to(DEV)


def _sew_check(got, q, k, attn_mod, geometry, what):
    """The kernel file's SEW bound for one map: fp64 O.sew_attention_core on the recorded u8 spikes q, k (T' * B_ * N1, C) in the
    reference's raw head view, with the attention module's table bias and scale and the shift mask of `geometry` = (D, H, W, ws, ss)."""
    D, H, W, ws, ss = geometry
    Tq, N1, nH = ws[0], ws[1] * ws[2], attn_mod.num_heads
    N = Tq * N1
    B_ = q.shape[0] // N
    assert got.shape == (B_, nH, N, N) and got.dtype == torch.float32
    idx = attn_mod.relative_position_index[:N, :N].reshape(-1).cpu()
    bias = attn_mod.relative_position_bias_table.detach().cpu().float()[idx].reshape(N, N, nH).permute(2, 0, 1).double()
    scale = float(torch.tensor(float(attn_mod.scale), dtype=torch.float32))      # the fp32 value the kernel reads
    mask = O.compute_mask(*_pad3(D, H, W, ws), ws, ss).double() if any(s > 0 for s in ss) else None
    view = lambda t: t.cpu().double().reshape(B_, nH, N, 32)
    _, a64 = O.sew_attention_core(view(q), view(k), view(k), scale, bias, mask, Tq, N1)
    S = (view(q) @ view(k).transpose(-2, -1)) * scale + bias.abs().unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        S = (S.view(B_ // nW, nW, nH, N, N) + mask.abs().view(1, nW, 1, N, N)).view(B_, nH, N, N)
    err = (got.cpu().double() - a64).abs()
    rel = (err / S.clamp(min=1e-300)).max().item()
    print(f"\nATTN_MAPS {what}: {tuple(got.shape)} max err / S {rel:.3e} (bound {SEW_REL:.3e}), max |a| {a64.abs().max().item():.3e}")
    assert bool((err <= SEW_REL * S).all()), rel


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_spikingformer_log_true_returns_the_maps_of_one_forward(kind):
    model = _sew_model(kind)
    x = harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=1234 + 7)).to(DEV)
    layers = model.sttmultires_unet.encoders.swin3d.layers
    plain = model(x)
    assert plain["attn"] is None
    with hip.launch_log() as log:
        out = model(x, log=True)
    assert all(torch.equal(a, b) for a, b in zip(out["flow"], plain["flow"])), "log=True changed the flows"
    assert sum(KERNEL in r[0] for r in log.rows) == len(layers) == len(out["attn"])
    # the same forward with the parity tape on: the q and k spikes of every attention, and the geometry each attention saw
    eng = model.engine()
    geometry, real = {}, eng.attention

    def spy(xs, blk, score_out=None):
        geometry[blk.name] = tuple(xs.shape[1:4]) + get_window_size(tuple(xs.shape[1:4]), blk.window_size, blk.shift_size)
        return real(xs, blk, score_out)
    eng.attention, eng.tape = spy, []
    try:
        taped = model(x, log=True)
        tape = {name: spikes for name, spikes, _ in eng.tape}
    finally:
        eng.tape = None
        del eng.attention
    assert all(torch.equal(a, b) for a, b in zip(taped["flow"], plain["flow"]))
    assert all(torch.equal(a, b) for a, b in zip(taped["attn"], out["attn"]))
    for s, (layer, m) in enumerate(zip(layers, taped["attn"])):
        name = f"sttmultires_unet.encoders.swin3d.layers.{s}.swin_blocks.{len(layer.swin_blocks) - 1}."
        q, k = tape[name + "attn.sn_q.spiking_neuron."], tape[name + "attn.sn_k.spiking_neuron."]
        _sew_check(m, q.view(-1, q.shape[-1]), k.view(-1, k.shape[-1]), layer.swin_blocks[-1].attn, geometry[name], f"SEW {kind} stage {s}")


@pytest.mark.parametrize("shift", [(0, 0, 0), (1, 4, 4)])
def test_sew_block_return_attention(shift):
    """Spiking_SwinTransformerBlock3D(x, None, return_attention=True): the map instead of the block's output, against the oracle's core
    on the block's own q and k spikes (the tape of the module's model-less engine).  20 x 25 -> 27 x 27 padded: padding tokens."""
    from sdformerflow_amd.STSwinNet_SNN import Spiking_swin_transformer3D as SW
    kw = {"num_steps": 4, "v_reset": None, "v_th": 0.1, "neuron_type": "lif", "surrogate_fun": "surrogate.ATan()", "tau": 2.0,
          "detach_reset": True, "spike_norm": "BN"}
    blk = SW.Spiking_SwinTransformerBlock3D(96, (20, 25), 3, window_size=(2, 9, 9), shift_size=shift, qk_scale=0.125, norm_layer="BN", **kw)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items() if not k.endswith(("relative_position_index",))})
    blk.load_state_dict(sd, strict=False)
    blk = blk.to(DEV).eval()
    x = ((rnd((1, 4, 20, 25, 96), 41) > 0.5).float() + (rnd((1, 4, 20, 25, 96), 42) > 0.7).float()).to(DEV)     # a sum of spike tensors
    eng, _ = module_forward._sew(blk)
    eng.tape = []
    try:
        with hip.launch_log() as log:
            got = blk(x, None, return_attention=True)
        tape = {name: spikes for name, spikes, _ in eng.tape}
    finally:
        eng.tape = None
    assert sum(KERNEL in r[0] for r in log.rows) == 1
    ws, ss = get_window_size((4, 20, 25), (2, 9, 9), shift)
    q, k = tape["attn.sn_q.spiking_neuron."], tape["attn.sn_k.spiking_neuron."]
    assert got.shape == (2 * 3 * 3, 3, 162, 162)
    _sew_check(got, q.view(-1, 96), k.view(-1, 96), blk.attn, (4, 20, 25, ws, ss), f"SEW block shift {shift}")
    out = blk(x, None)                                                               # the plain forward is what it was
    assert out.shape == x.shape


def test_sew_refusals_happen_before_any_launch():
    model = _sew_model("lif")
    x = harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=1234 + 7)).to(DEV)
    blk = model.sttmultires_unet.encoders.swin3d.layers[0].swin_blocks[-1]
    model.train()
    try:
        with hip.launch_log() as log, pytest.raises(NotImplementedError, match="eval mode"):
            model(x, log=True)
        assert not log.rows, log.rows
        with hip.launch_log() as log, pytest.raises(NotImplementedError):
            blk(torch.zeros(1, 4, 36, 48, 96, device=DEV), None, return_attention=True)
        assert not log.rows, log.rows
    finally:
        model.eval()
