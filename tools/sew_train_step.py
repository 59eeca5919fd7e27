#!/usr/bin/env python3
"""Time one training step of the SEW SpikingformerFlowNet (configs/train_DSEC_supervised_SDformerFlow_en4.yml with the SEW class,
288 x 384, local batch 4), fp32 and under bf16 autocast, with the HIP attention backward (csrc/win_attn_sew_bwd.hip) and with
SDF_SEW_ATTN_BWD=0 (the attention core as a torch composition that keeps the (B_, nH, N, N) scores) in the same process.  Also reports
the attention backward's kernel time per step (library launch log, one fp32 step) split into its three kernels, and its fraction of the
fp32 roof: per (window, head) 10 N 32^2 (Grams, dq, dk, the Gram part of dv) + 4 N^2 32 (the (bias + mask)^T dO term and d_bias) FLOP.

    python tools/sew_train_step.py [--batch 4] [--steps 10] [--warmup 3]

Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import yaml  # noqa: E402

from sdformerflow_amd import harness, hip, train  # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

CFG = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
FP32_PEAK = 157.3e12               # MI355X fp32, vector (v_pk_fma_f32) and matrix alike (MI355X_MICROARCH)


def build(H, W):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"].update(input_size=[H, W], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    net = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()
                                          if not k.endswith(("relative_position_index", "num_batches_tracked"))}), strict=False)
    return net.cuda().train()


def attn_flops(net, B, H, W):
    """Backward FLOP of the attention core over every block of every stage (padded maps, D = 10 time steps)."""
    D, h, w = 10, H // 4, W // 4
    total = 0
    for layer in net.sttmultires_unet.encoders.swin3d.layers:
        for blk in layer.swin_blocks:
            (wd, wh, ww), _ = train.get_window_size((D, h, w), blk.window_size, blk.shift_size)
            nwin = B * -(-D // wd) * -(-h // wh) * -(-w // ww)
            N = wd * wh * ww
            total += nwin * blk.attn.num_heads * (10 * N * 32 * 32 + 4 * N * N * 32)
        h, w = -(-h // 2), -(-w // 2)
    return total


def step_ms(net, opt, chunk, label, mask, steps, warmup, amp):
    buckets = train.GradientBuckets(net.parameters())
    for _ in range(warmup):
        train.train_step(net, opt, chunk, label, mask, buckets=buckets, amp=amp)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = train.train_step(net, opt, chunk, label, mask, buckets=buckets, amp=amp)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=288)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    B, H, W = a.batch, a.height, a.width
    net = build(H, W)
    chunk = harness.prepare_chunk(synth_voxel(B, 10, H, W, seed=910)).cuda()
    label, mask = (t.cuda() for t in synth_label(B, H, W, seed=911))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-5, weight_decay=0.01)
    res = {"model": "SpikingformerFlowNet", "batch": B, "size": [H, W]}
    for amp in (False, True):
        tag = "bf16" if amp else "fp32"
        torch.cuda.reset_peak_memory_stats()
        res[f"step_ms_{tag}"], res[f"loss_{tag}"] = step_ms(net, opt, chunk, label, mask, a.steps, a.warmup, amp)
        res[f"peak_mem_gib_{tag}"] = torch.cuda.max_memory_allocated() / 2 ** 30
        with hip.scoped_switches(SDF_SEW_ATTN_BWD="0"):
            torch.cuda.reset_peak_memory_stats()
            res[f"step_ms_{tag}_torch_attn"], res[f"loss_{tag}_torch_attn"] = step_ms(net, opt, chunk, label, mask, a.steps, a.warmup, amp)
            res[f"peak_mem_gib_{tag}_torch_attn"] = torch.cuda.max_memory_allocated() / 2 ** 30
    torch.cuda.synchronize()
    with hip.launch_log() as log:
        train.train_step(net, opt, chunk, label, mask)
        torch.cuda.synchronize()
    bwd = [r for r in log.rows if "sew_bwd" in r[0]]
    res["attn_bwd_launches"] = len(bwd)
    res["attn_bwd_kernel_ms"] = sum(r[4] for r in bwd) / 1e3
    part = lambda name: "dbias_finish" if "dbias_finish" in name else "dbias" if "dbias" in name else "main"
    for p in ("main", "dbias", "dbias_finish"):
        res[f"attn_bwd_{p}_ms"] = sum(r[4] for r in bwd if part(r[0]) == p) / 1e3
    res["attn_bwd_kernel_names"] = sorted({r[0] for r in bwd})
    fwd = [r for r in log.rows if "win_attn" in r[0] and "sew_bwd" not in r[0]]
    res["attn_fwd_kernel_ms"] = sum(r[4] for r in fwd) / 1e3
    flops = attn_flops(net, B, H, W)
    res["attn_bwd_gflop"] = flops / 1e9
    res["attn_bwd_fp32_roof_ms"] = flops / FP32_PEAK * 1e3
    res["attn_bwd_roof_fraction"] = res["attn_bwd_fp32_roof_ms"] / res["attn_bwd_kernel_ms"] if bwd else None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
