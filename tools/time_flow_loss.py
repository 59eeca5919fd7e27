#!/usr/bin/env python3
"""The training step's head on one MI355X: train.flow_loss_hip (hip.flow_loss, csrc/flow_loss.hip, autograd.FlowLossFunction) against
the torch composition it is the opt-in twin of - `pred.sum(0)`, F.interpolate and train.flow_loss_supervised with autograd - same
process, alternating legs, median of the rounds.

Workload: the en4 training shape - local batch 4, 288 x 384 - with the raw predictions one train-mode forward of the en4 model makes
(train.forward_train_preds: the model's own levels and T; synthetic weights, seeded input), detached, so that only the head is timed:
forward from the raw predictions to the loss plus backward to the predictions' gradients.  Times are device time between two HIP events
around `iters` back-to-back forward + backward calls.  Launches of one call: every device kernel torch's profiler records, and for the
HIP head the library's own launch log beside it.  Peak memory: torch.cuda.max_memory_allocated over one call above what is allocated
before it.  Both legs' values are compared first.

    python tools/time_flow_loss.py --out profiles/flow_loss_timing.txt
"""
import argparse
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL_NAME = re.compile(r"(\w+)(?:<.*?>)?\(")          # `flow_loss_partial_kernel` of the launch log's demangled signature


def event_us(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def device_kernels(fn):
    """Names of the device kernels of one call of fn, from torch's profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = []
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
            names.append(e.name)
    return names


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X (no CPU fallback)"
    import yaml
    from sdformerflow_amd import hip, train
    from sdformerflow_amd.harness import prepare_chunk
    from sdformerflow_amd.spikingjelly_compat import functional
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4
    from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, H, W = args.batch, 288, 384
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"]["input_size"] = [H, W]
    model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model.to(dev).train()
    functional.reset_net(model)
    chunk = prepare_chunk(synth_voxel(B, 10, H, W, seed=1238)).to(dev)
    label, mask = (t.to(dev) for t in synth_label(B, H, W))
    with torch.no_grad():
        preds = [p.detach().clone() for p in train.forward_train_preds(model, chunk)]
    del model
    torch.cuda.empty_cache()
    n = train.global_valid_count(mask)
    fs, lam = float(cfg["metrics"]["flow_scaling"]), float(cfg["loss"]["lambda_mod"])
    say(f"time_flow_loss: {torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, flow_scaling {fs}, lambda_mod {lam}; levels (T, B, 2, h, w): "
        + ", ".join(str(tuple(p.shape)) for p in preds) + f"; {args.iters} calls per window, {args.rounds} rounds, legs alternating")
    leaves = [p.requires_grad_(True) for p in preds]

    def torch_head():
        for p in leaves:
            p.grad = None
        flows = train._flows_of_preds(leaves, H, W)
        train.flow_loss_supervised([f.float() for f in flows], label, mask, fs, lam, n_valid=n).backward()

    def hip_head():
        for p in leaves:
            p.grad = None
        train.flow_loss_hip(leaves, label, mask, fs, lam, n_valid=n).backward()

    torch_head()
    want = [p.grad.clone() for p in leaves]
    with torch.no_grad():
        t_loss = float(train.flow_loss_supervised([f.float() for f in train._flows_of_preds(preds, H, W)], label, mask, fs, lam, n_valid=n))
    hip_head()
    h_loss = float(hip.flow_loss([p.detach() for p in preds], label, mask.float(), n.reshape(1), fs, lam, grads=False)[0])
    worst = max(float((p.grad - g).abs().max() / g.abs().max()) for p, g in zip(leaves, want))
    say(f"loss: torch {t_loss!r}, hip {h_loss!r}; largest gradient difference over a level's largest element {worst:.2e}")

    legs = {"hip": hip_head, "torch": torch_head}
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(event_us(fn, args.iters))
    say()
    say("device time of the head, forward + backward, between two events around back-to-back calls, us: median (min .. max of the rounds)")
    for k, v in times.items():
        say(f"  {k:6s} {statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})")
    ratio = statistics.median(times["torch"]) / statistics.median(times["hip"])
    say(f"  torch / hip = {ratio:.2f}" + ("" if ratio > 1 else "   THE HIP HEAD IS NOT FASTER THAN THE TORCH HEAD IN THIS RUN"))

    say()
    say("device kernels of one forward + backward (torch's profiler), and peak memory of one call above the allocation before it")
    for k, fn in legs.items():
        names = device_kernels(fn)
        say(f"  {k:6s} {len(names):4d} kernels   peak {peak_bytes(fn) / 2 ** 20:8.1f} MiB")
    with hip.launch_log() as log:
        hip_head()
    torch.cuda.synchronize()
    say("  the HIP head's library launches (launch log, events around each launch): "
        + ", ".join(f"{KERNEL_NAME.search(r[0]).group(1)} {r[1]} x {r[2]} {r[4]:.1f} us" for r in log.rows))
    moved = B * H * W * 12 + sum(p.numel() * p.element_size() + p[0].numel() * 4 for p in preds)
    part = [r[4] for r in log.rows if "partial" in r[0]]
    if part:
        say(f"  algorithmic minimum of the partial launch: label, mask, predictions read once, gradients written once = {moved / 1e6:.1f} MB "
            f"-> {moved / part[0] / 1e6:.2f} TB/s")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
