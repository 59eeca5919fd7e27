#!/usr/bin/env python3
"""Time one training step of the 240 x 240, three-stage (depths [2,2,6]) STTFlowNet (ANN) and SpikingformerFlowNet (SEW) at window
(2,15,15) - 450 tokens per window - with the HIP attention both ways (SDF_*_ATTN_BWD=2: csrc/win_attn_large.hip forward,
csrc/win_attn_large_bwd.hip backward) and with the torch composition of the attention (=0), in one process: the two routes alternate in
blocks of steps after a warm-up of each, every step is timed with device events, and the median step time and the peak of
torch.cuda.max_memory_allocated() of each route are reported side by side.  One further step of the HIP route runs under the
library's launch log for the per-kernel times of the attention kernels, set against the FLOPs the backward needs (computed from the
shapes) at the 157.3 TFLOPS exact-fp32 MFMA / fp32 vector rate.

    python tools/large_window_train_measure.py [--batch 1] [--steps 8] [--rounds 3] [--warmup 3] [--out profiles/large_window_train.txt]

Needs a GPU (no fallback)."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import yaml  # noqa: E402

from sdformerflow_amd import harness, hip, train  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

FP32_PEAK = 157.3e12               # MI355X: v_mfma_f32_16x16x4_f32 and the fp32 vector ALU alike (MI355X_MICROARCH)
WS, PWS, SIZE = (2, 15, 15), (2, 9, 9), (240, 240)
N, HEADS, BLOCKS, MAPS = 450, (3, 6, 12), (2, 2, 6), (60, 30, 15)
# products of 2 N^2 32 FLOP per (window, head): ANN - Q K^T and V dO^T in each of the two query walks, the key walk and the d_bias
# kernel (8), dS K^, P^T dO, dS^T Q^ (3); SEW - (bias + mask)^T dO and dO V^T (2; the Gram products are O(N 32^2))
PRODUCTS = {"ann": 11, "sew": 2}
FORWARD = "win_attn_large_kernel"


def build(family):
    cfgs = os.path.join(ROOT, "sdformerflow_amd", "configs")
    if family == "ann":
        from sdformerflow_amd.STSwinNet import STSwinNet
        cfg = yaml.safe_load(open(os.path.join(cfgs, "train_DSEC_supervised_STT_voxel.yml")))
        swin = dict(cfg["swin_transformer"], input_size=list(SIZE), window_size=list(WS), pretrained_window_size=list(PWS))
        net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), swin)
        net.norm_input = False
        skip = ("relative_position_index", "relative_coords_table", "num_batches_tracked")
    else:
        from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
        cfg = yaml.safe_load(open(os.path.join(cfgs, "train_DSEC_supervised_SDformerFlow_en4.yml")))
        cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
        cfg["swin_transformer"].update(input_size=list(SIZE), window_size=list(WS), swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12],
                                       swin_out_indices=[0, 1, 2])
        net = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
        skip = ("relative_position_index",)
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(skip)}), strict=False)
    return net.cuda()


def windows(batch, depth):
    """(windows, heads) of every block: the stage maps of 60, 30 and 15 padded to multiples of 15"""
    return [(batch * -(-depth // WS[0]) * (-(-m // 15)) ** 2, h) for m, h, n in zip(MAPS, HEADS, BLOCKS) for _ in range(n)]


def timed_steps(step, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def measure(family, a, say):
    switch = "SDF_ANN_ATTN_BWD" if family == "ann" else "SDF_SEW_ATTN_BWD"
    torch.manual_seed(0)
    net = build(family)
    bins = 20 if family == "ann" else 10
    vox = synth_voxel(a.batch, bins, *SIZE, seed=808)
    chunk = (vox if family == "ann" else harness.prepare_chunk(vox)).cuda()
    label, mask = (t.cuda() for t in synth_label(a.batch, *SIZE, seed=809))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=0.01)
    step = lambda: train.train_step(net, opt, chunk, label, mask, clip_grad=None)
    times, peak = {"2": [], "0": []}, {"2": 0, "0": 0}
    for value in ("2", "0"):                                   # every shape of both routes once before anything is timed
        with hip.scoped_switches(**{switch: value}):
            for _ in range(a.warmup):
                step()
    torch.cuda.synchronize()
    for _ in range(a.rounds):                                  # the routes alternate: drift of a shared machine hits both alike
        for value in ("2", "0"):
            with hip.scoped_switches(**{switch: value}):
                torch.cuda.reset_peak_memory_stats()
                times[value] += timed_steps(step, a.steps)
                peak[value] = max(peak[value], torch.cuda.max_memory_allocated())
    with hip.scoped_switches(**{switch: "2"}), hip.launch_log() as log:
        step()
        torch.cuda.synchronize()
    wins = windows(a.batch, 2)                                 # the stage maps are two tokens deep: one window
    flops = sum(w * h * PRODUCTS[family] * 2 * N * N * 32 for w, h in wins)
    say(f"== {family.upper()} model, batch {a.batch}, {SIZE[0]} x {SIZE[1]}, window {WS} ({N} tokens), {sum(BLOCKS)} blocks, "
        f"{sum(w * h for w, h in wins)} (window, head) pairs per step ==")
    say(f"{'route':<34}{'median step ms':>16}{'min':>9}{'max':>9}{'steps':>7}{'peak allocated MiB':>20}")
    for value, name in (("2", f"{switch}=2 (HIP both ways)"), ("0", f"{switch}=0 (torch composition)")):
        t = times[value]
        say(f"{name:<34}{statistics.median(t):>16.2f}{min(t):>9.2f}{max(t):>9.2f}{len(t):>7}{peak[value] / 2 ** 20:>20.1f}")
    say("attention kernels of one step under =2 (library launch log: launches, total microseconds):")
    kern = {}
    for name, _, _, _, us in log.rows:
        if "win_attn" in name:
            short = re.sub(r"[<(].*$", "", name.replace("void ", "").replace("(anonymous namespace)::", ""))
            n, t = kern.get(short, (0, 0.0))
            kern[short] = (n + 1, t + us)
    for name, (n, t) in kern.items():
        say(f"    {name:<48}{n:>5}{t:>12.1f}")
    bwd_us = sum(t for name, (n, t) in kern.items() if name != FORWARD)
    roof_us = flops / FP32_PEAK * 1e6
    say(f"backward: {flops / 1e9:.2f} GFLOP ({PRODUCTS[family]} products of 2 N^2 32 per (window, head)), {roof_us:.1f} us at {FP32_PEAK / 1e12:.1f} "
        f"TFLOPS; kernels {bwd_us:.1f} us = {roof_us / bwd_us:.1%} of that rate" if bwd_us else "backward: no kernel logged")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_window_train.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("large_window_train_measure needs a GPU: nothing is measured without one")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"tools/large_window_train_measure.py --batch {a.batch} --steps {a.steps} --rounds {a.rounds} --warmup {a.warmup}")
    say(f"device: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}); one process, routes alternating in blocks of {a.steps} steps, device-event time per step")
    say("")
    for family in ("ann", "sew"):
        measure(family, a, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
