#!/usr/bin/env python3
"""Time one training step of the ANN STTFlowNet (BASELINE configs[2]: STT_voxel config, B = 8, 288 x 384): train-mode forward,
backward and AdamW, with the fused attention backward (csrc/win_attn_bwd.hip) and with SDF_ANN_ATTN_BWD=0 (the attention as a
torch composition) in the same process.  Also reports the attention backward's own kernel time (library launch log, one step) and
its fraction of the fp32-MFMA roof: 5 products x 2 N^2 32 FLOP per (window, head).

    python tools/ann_train_step.py [--batch 8] [--steps 10] [--warmup 3]

Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import yaml  # noqa: E402

from sdformerflow_amd import hip, train  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

FP32_MFMA_PEAK = 157.3e12          # MI355X, v_mfma_f32_16x16x4_f32 (MI355X_MICROARCH: 155 TF measured)


def build(H, W):
    from sdformerflow_amd.STSwinNet import STSwinNet
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")))
    net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), dict(cfg["swin_transformer"], input_size=[H, W]))
    skip = ("relative_position_index", "relative_coords_table", "num_batches_tracked")
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(skip)}), strict=False)
    return net.cuda()


def attn_flops(net, B, H, W):
    """5 products x 2 N^2 32 per (window, head), every block of every stage (padded maps)."""
    from sdformerflow_amd.STSwinNet.swin_transformer3D_v2 import SwinTransformerBlock3D
    D, h, w = net.num_bins // 10, H // 4, W // 4
    total = 0
    for layer in net.sttmultires_unet.encoders.swin3d.layers:
        for blk in layer.swin_blocks:
            ws = blk.window_size
            nwin = B * -(-D // ws[0]) * -(-h // ws[1]) * -(-w // ws[2])
            N = ws[0] * ws[1] * ws[2]
            total += nwin * blk.num_heads * 5 * 2 * N * N * 32
            assert isinstance(blk, SwinTransformerBlock3D)
        h, w = -(-h // 2), -(-w // 2)
    return total


def step_ms(net, opt, vox, label, mask, steps, warmup):
    for _ in range(warmup):
        train.train_step(net, opt, vox, label, mask, clip_grad=None)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = train.train_step(net, opt, vox, label, mask, clip_grad=None)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    B, H, W = a.batch, a.height, a.width
    net = build(H, W)
    vox = synth_voxel(B, 20, H, W, seed=808).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=809))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.01)
    res = {"model": "STTFlowNet", "batch": B, "size": [H, W]}
    res["step_ms"], res["loss"] = step_ms(net, opt, vox, label, mask, a.steps, a.warmup)
    torch.cuda.synchronize()
    with hip.launch_log() as log:
        train.train_step(net, opt, vox, label, mask, clip_grad=None)
        torch.cuda.synchronize()
    bwd = [r for r in log.rows if "win_attn_ann_bwd" in r[0]]
    res["attn_bwd_launches"] = len(bwd)
    res["attn_bwd_kernel_ms"] = sum(r[4] for r in bwd) / 1e3
    res["attn_bwd_main_ms"] = sum(r[4] for r in bwd if "reduce" not in r[0]) / 1e3
    flops = attn_flops(net, B, H, W)
    res["attn_bwd_gflop"] = flops / 1e9
    res["attn_bwd_fp32_mfma_roof_ms"] = flops / FP32_MFMA_PEAK * 1e3
    res["attn_bwd_roof_fraction"] = res["attn_bwd_fp32_mfma_roof_ms"] / res["attn_bwd_kernel_ms"] if bwd else None
    res["peak_mem_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    with hip.scoped_switches(SDF_ANN_ATTN_BWD="0"):                       # A/B: the attention as a torch composition
        torch.cuda.reset_peak_memory_stats()
        res["step_ms_torch_attn"], res["loss_torch_attn"] = step_ms(net, opt, vox, label, mask, a.steps, a.warmup)
        res["peak_mem_gib_torch_attn"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(res))


if __name__ == "__main__":
    main()
