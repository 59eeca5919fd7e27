#!/usr/bin/env python3
"""The training front end on one MI355X: train.prepare_train_item (hip.augment_chunk, csrc/prepare_chunk.hip) against the torch
composition it replaces (train.prepare_train_item_torch: the transforms of DSEC_dataloader.data_augmentation, harness.prepare_chunk,
the event-mask product), same process, alternating legs, median of the rounds.

Workload: the en4 training shape - local batch 4, the config's bins, a 480 x 640 loader item (synthetic.synth_voxel / synth_label),
RandomCrop(288, 384) and both flips at p = 0.5, min-max - without a drop and with Random_event_drop at p = 1.  Times are device time
between two HIP events around `iters` back-to-back calls (the host's own time shows where it stalls the queue: the torch legs wait
for the device inside every call); the kernel's two launches are also timed one by one through the library's launch log.  The host
synchronisations of a call are counted with torch.cuda.set_sync_debug_mode("warn").  Bytes: the algorithmic minimum - the window read
once; input, label and mask written once; the finish's read-modify-write of the input - over the kernel time.

    python tools/augment_chunk_measure.py --out profiles/augment_chunk_timing.txt
"""
import argparse
import os
import random
import re
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # spec; a float4 copy's measured rate


def event_us(fn, iters, warm=5):
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


def host_syncs(fn):
    """Synchronising calls torch reports for one call of fn (None where the debug mode reports nothing at all for a known one)."""
    def count(f):
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                f()
            return sum("synchroniz" in str(m.message).lower() for m in w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    if count(lambda: torch.ones(1, device="cuda").item()) == 0:
        return None
    return count(fn)


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
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    B, bins, (Hs, Ws), (h, w) = args.batch, int(cfg["model"]["num_bins"]), (480, 640), tuple(cfg["loader"]["crop"])
    cfg["metrics"]["mask_events"] = False
    vox = synth_voxel(B, bins, Hs, Ws, seed=1238).to(dev)
    label, mask = (t.to(dev) for t in synth_label(B, Hs, Ws))
    p = cfg["loader"]["augment_prob"]
    chains = {"no drop": train.train_transform(cfg),
              "drop": D.Compose([D.RandomCrop((h, w)), D.Random_horizontal_flip(p[0]), D.Random_vertical_flip(p[1]),
                                 D.Random_event_drop(0.0, 0.6, p=1.0)])}
    say(f"augment_chunk_measure: {torch.cuda.get_device_name(0)}; batch {B}, {bins} bins, {Hs} x {Ws} -> {h} x {w}, norm_input "
        f"{cfg['model']['norm_input']}, spike_th {cfg['data']['spike_th']}, mask_events off; {args.iters} calls per window, {args.rounds} "
        f"rounds, legs alternating; the draws differ from call to call (RandomCrop, flips p = {p[0]}, {p[1]})")

    # the two sides agree on this input (the drop's field handed to both)
    for name, t in chains.items():
        u = torch.rand((B, bins, h, w), device=dev)
        random.seed(5), torch.manual_seed(5)
        prm = t.sample(vox.shape)
        got = hip.augment_chunk(vox, label, mask, prm.crop, *prm.per_sample(B), drop_u=u, norm_input="minmax")
        random.seed(5), torch.manual_seed(5)
        want = train.prepare_train_item_torch(vox, label, mask, cfg, t, drop_u=u)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), name
    say("outputs of both sides are equal on this input (x, label, mask; the drop's uniform field given to both)")

    step = [0]

    def hip_leg(t):
        def call():
            step[0] += 1
            return train.prepare_train_item(vox, label, mask, cfg, t, step=step[0])
        return call
    legs = {}
    for name, t in chains.items():
        legs[f"hip, {name}"] = hip_leg(t)
        legs[f"torch, {name}"] = (lambda t: lambda: train.prepare_train_item_torch(vox, label, mask, cfg, t))(t)
    random.seed(0), torch.manual_seed(0)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(event_us(fn, args.iters if k.startswith("hip") else max(args.iters // 4, 10)))
    say()
    say("device time per call between two events around back-to-back calls, us: median (min .. max of the rounds); host synchronisations per call")
    for k, v in times.items():
        n = host_syncs(legs[k])
        say(f"  {k:16s} {statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})   syncs {'not reported by the debug mode' if n is None else n}")
    for name in chains:
        a, b = statistics.median(times[f"hip, {name}"]), statistics.median(times[f"torch, {name}"])
        say(f"  {name}: torch / hip = {b / a:.1f}")

    # the launches one by one, and the bytes
    say()
    say("the kernel's launches (library launch log, events around each launch; median of 50 calls), and the algorithmic minimum of bytes")
    cells = B * h * w
    gather = cells * 4 * (bins + 2 + 1) + cells * 4 * (2 * bins + 2 + 1)          # the window read once | input, label, mask written once
    finish = cells * 4 * 2 * bins * 2                                            # read-modify-write of the input
    for name, t in chains.items():
        rows = {}
        for i in range(55):
            with hip.launch_log() as log:
                legs[f"hip, {name}"]()
            torch.cuda.synchronize()
            if i >= 5:
                for r in log.rows:
                    rows.setdefault(re.search(r"(\w+)(?:<.*?>)?\(", r[0]).group(1), []).append(r[4])
        total = 0.0
        for kernel, us in rows.items():
            med = statistics.median(us)
            total += med
            nbytes = gather if "augment" in kernel else finish
            say(f"  {name:8s} {kernel:24s} {med:8.1f} us   {nbytes / 1e6:7.1f} MB minimum -> {nbytes / med / 1e6:7.2f} TB/s "
                f"({100 * nbytes / med / 1e-6 / HBM_COPY:.0f} % of a copy's {HBM_COPY / 1e12:.2f} TB/s, {100 * nbytes / med / 1e-6 / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s spec)")
        say(f"  {name:8s} both launches {total:8.1f} us for {(gather + finish) / 1e6:.1f} MB: {(gather + finish) / total / 1e6:.2f} TB/s; a single pass "
            f"over the minimum without the finish's re-read would move {(gather) / 1e6:.1f} MB")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
