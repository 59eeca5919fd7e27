#!/usr/bin/env python3
"""Time one training step of the en4 MS model (configs/train_DSEC_supervised_SDformerFlow_en4.yml, 288 x 384, local batch 4) with
`neuron_type: lif` and `plif` in the same process, same synthetic weights and inputs, fp32 and under bf16 autocast; and the neuron
backward kernels on the same tensor (the stage-0 hidden tensor, T = 10): sdf_plif_bwd (dL/dx and dL/dk) against sdf_lif_bwd.

    python tools/plif_train_step.py [--batch 4] [--steps 10] [--warmup 3]

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
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

CFG = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")


def build(kind, H, W):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"]["input_size"] = [H, W]
    net = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}), strict=True)
    return net.cuda().train()


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


def kernel_us(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    H, W = 288, 384
    out = {"shape": [a.batch, H, W]}
    # kernels: T = 10 x 69 120 x 384 (the stage-0 hidden tensor at local batch 4), x and dL/ds in, dL/dx out (+ one partial per workgroup)
    T, N = 10, 6912 * 384
    x = torch.rand((T, N), device="cuda") * 0.6 - 0.3
    g = torch.randn((T, N), device="cuda")
    k = torch.sigmoid(torch.tensor([0.35], device="cuda"))
    out["lif_bwd_us"] = kernel_us(lambda: hip.lif_bwd(x, g, 2.0, 0.1, None, True, 2.0))
    out["plif_bwd_us"] = kernel_us(lambda: hip.plif_bwd(x, k, g, 0.1, None, True, 2.0))
    out["plif_over_lif_bwd"] = out["plif_bwd_us"] / out["lif_bwd_us"]
    out["plif_bwd_TBps"] = T * N * 12 / out["plif_bwd_us"] / 1e6
    if not a.kernels_only:
        chunk = harness.prepare_chunk(synth_voxel(a.batch, 10, H, W, seed=7)).cuda()
        label, mask = synth_label(a.batch, H, W, seed=8)
        label, mask = label.cuda(), mask.cuda()
        for amp in (False, True):
            for kind in ("lif", "plif"):
                torch.manual_seed(0)
                net = build(kind, H, W)
                opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.01)
                ms, loss = step_ms(net, opt, chunk, label, mask, a.steps, a.warmup, amp)
                out[f"{kind}_{'bf16' if amp else 'fp32'}_step_ms"], out[f"{kind}_{'bf16' if amp else 'fp32'}_loss"] = ms, loss
                del net, opt
                torch.cuda.empty_cache()
            tag = "bf16" if amp else "fp32"
            out[f"plif_over_lif_{tag}"] = out[f"plif_{tag}_step_ms"] / out[f"lif_{tag}_step_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
