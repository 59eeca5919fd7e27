#!/usr/bin/env python3
"""The MDR training front end on one MI355X: train.prepare_mdr_item (hip.augment_resize_chunk, csrc/prepare_chunk.hip) against the torch
sequence it is compared with (train.prepare_mdr_item_torch: per-sample index gathers, harness.prepare_chunk, the event-mask product),
same process, alternating legs, median of the rounds.

Workload: the MDR configuration's own shape - local batch 4, 2 x 10 bins, a 260 x 346 item (synthetic.synth_voxel / synth_label),
DenseSparseAugmentor([256, 256], min_scale -0.2, max_scale 0.5, do_flip=True), min-max - with ONE batch of records drawn under a
fixed seed (numpy seed 0) and used by every call of both legs, so that both sides do the same work.  Times are device time between two
HIP events around `iters` back-to-back calls; the kernel's launches are also timed one by one through the library's launch log.  The
host synchronisations of a call are counted with torch.cuda.set_sync_debug_mode("warn").  Bytes: the algorithmic minimum - the window
of the source a sample's crop maps to read once; input, label and mask written once; the finish's read-modify-write of the input -
over the kernel time, beside a device-to-device copy of as many bytes timed in the same run.  The reference's own path - cv2.resize on
the host, per sample, in the loader's workers - cannot be timed here: cv2 is not available.

    python tools/mdr_augment_measure.py --out profiles/mdr_augment_timing.txt
"""
import argparse
import os
import re
import statistics
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12          # spec


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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X (no CPU fallback)"
    from sdformerflow_amd import hip, train
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, bins, (Hs, Ws), (h, w) = args.batch, 10, (260, 346), (256, 256)
    cfg = {"model": {"norm_input": "minmax", "encoding": "voxel"}, "data": {"num_chunks": 2, "spike_th": None},
           "loader": {"polarity": True, "crop": [h, w], "min_scale": -0.2, "max_scale": 0.5}, "metrics": {"mask_events": False}}
    sample = {"d_event_volume_old": synth_voxel(B, bins, Hs, Ws, seed=1301).to(dev),
              "d_event_volume_new": synth_voxel(B, bins, Hs, Ws, seed=1302).to(dev), "flow": synth_label(B, Hs, Ws)[0].to(dev)}
    aug = train.mdr_train_augmentor(cfg)
    np.random.seed(args.seed)
    params = aug.sample_batch(B, (Hs, Ws))
    nF = 2 * bins
    say(f"mdr_augment_measure: {torch.cuda.get_device_name(0)}; batch {B}, 2 x {bins} bins, {Hs} x {Ws} -> {h} x {w}, norm_input minmax, "
        f"spike_th None, mask_events off; {args.iters} calls per window, {args.rounds} rounds, legs alternating; records of numpy seed {args.seed}:")
    for p in params:
        say(f"  {p}")

    got = train.prepare_mdr_item(sample, cfg, aug, params)
    want = train.prepare_mdr_item_torch(sample, cfg, aug, params)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    say("outputs of both sides are equal on this input (x, label, mask)")

    legs = {"hip": lambda: train.prepare_mdr_item(sample, cfg, aug, params),
            "torch": lambda: train.prepare_mdr_item_torch(sample, cfg, aug, params)}
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            times[k].append(event_us(fn, args.iters if k == "hip" else max(args.iters // 10, 10)))
    say()
    say("device time per call between two events around back-to-back calls, us: median (min .. max of the rounds); host synchronisations per call")
    for k, v in times.items():
        n = host_syncs(legs[k])
        say(f"  {k:8s} {statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})   syncs {'not reported by the debug mode' if n is None else n}")
    say(f"  torch / hip = {statistics.median(times['torch']) / statistics.median(times['hip']):.1f}")

    # the launches one by one, and the bytes: a resized sample's crop maps to a window of h / scale_y x w / scale_x source pixels
    say()
    say("the kernel's launches (library launch log, events around each launch; median of 50 calls), and the algorithmic minimum of bytes")
    src = sum((h / p.scale_y) * (w / p.scale_x) if p.resized else h * w for p in params)
    cells = B * h * w
    gather = int(src * 4 * (nF + 2) + cells * 4 * (2 * nF + 2 + 1))               # the source windows read once | input, label, mask written once
    finish = cells * 4 * 2 * nF * 2                                             # read-modify-write of the input
    rows = {}
    for i in range(55):
        with hip.launch_log() as log:
            legs["hip"]()
        torch.cuda.synchronize()
        if i >= 5:
            for r in log.rows:
                rows.setdefault(re.search(r"(\w+)(?:<.*?>)?\(", r[0]).group(1), []).append(r[4])
    total = 0.0
    for kernel, us in rows.items():
        med = statistics.median(us)
        total += med
        nbytes = gather if "augment" in kernel else finish
        say(f"  {kernel:24s} {med:8.1f} us   {nbytes / 1e6:7.1f} MB minimum -> {nbytes / med / 1e6:7.2f} TB/s ({100 * nbytes / med / 1e-6 / HBM_PEAK:.0f} % of the "
            f"{HBM_PEAK / 1e12:.0f} TB/s spec)")
    say(f"  both launches {total:8.1f} us for {(gather + finish) / 1e6:.1f} MB: {(gather + finish) / total / 1e6:.2f} TB/s")
    # a copy of as many bytes, in the same run (read + write = the bytes moved)
    for name, nbytes in (("the gather's", gather), ("both launches'", gather + finish)):
        a = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        us = statistics.median(event_us(lambda: b.copy_(a), 200) for _ in range(5))
        say(f"  a device-to-device copy moving {name} {2 * a.numel() * 4 / 1e6:.1f} MB: {us:.1f} us, {2 * a.numel() * 4 / us / 1e6:.2f} TB/s")
    say("the reference's host path (cv2.resize per sample in the loader's workers) is not timed: cv2 is not available")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
