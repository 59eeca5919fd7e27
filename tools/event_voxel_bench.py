#!/usr/bin/env python3
"""Time the event front end on one MI355X, in one process: (i) the torch composition a user has without it - the reference's
convert_CHW restated on GPU tensors (eight put_(accumulate=True) passes, event_representations.py:248-277), centre crop, polarity
split and min-max (harness.prepare_chunk) - against (ii) harness.events_to_chunk (HIP), for N = 1e5, 1e6, 4e6 events at 10 bins,
480 x 640 -> 288 x 384.  Device events around `reps` back-to-back calls after warm-up, the two legs alternating, median of `rounds`;
the HIP leg is also split into its stages (keys | torch stable sort | gather) from the library's launch log and a sort-only timing.

    python tools/event_voxel_bench.py [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdformerflow_amd import harness, hip  # noqa: E402

SENSOR, CROP, BINS = (480, 640), (288, 384), 10


def torch_convert_chw(ev, C, H, W):
    grid = torch.zeros((C, H, W), dtype=torch.float32, device=ev["t"].device)
    t = ev["t"]
    tn = (C - 1) * (t - t[0]) / (t[-1] - t[0])
    x0, y0, t0 = ev["x"].int(), ev["y"].int(), tn.int()
    value = 2 * ev["p"] - 1
    for xl in (x0, x0 + 1):
        for yl in (y0, y0 + 1):
            for tl in (t0, t0 + 1):
                keep = (xl < W) & (xl >= 0) & (yl < H) & (yl >= 0) & (tl >= 0) & (tl < C)
                wgt = value * (1 - (xl - ev["x"]).abs()) * (1 - (yl - ev["y"]).abs()) * (1 - (tl - tn).abs())
                grid.put_((H * W * tl.long() + W * yl.long() + xl.long())[keep], wgt[keep], accumulate=True)
    return grid


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from test_event_voxel_gpu import synth_events
    lines = [f"event front end, {BINS} bins, {SENSOR} -> {CROP}, minmax; ms per call, median of {a.rounds} rounds x {a.reps} calls ({torch.cuda.get_device_name(0)})"]
    for n in (100000, 1000000, 4000000):
        ev = {k: torch.from_numpy(v).cuda() for k, v in synth_events(n, seed=3).items()}
        legs = {"torch": lambda: harness.prepare_chunk(harness.center_crop(torch_convert_chw(ev, BINS, *SENSOR)[None], CROP), "minmax"),
                "hip": lambda: harness.events_to_chunk(ev, BINS, SENSOR, CROP, "minmax", None),
                "hip_nocheck": lambda: hip.event_voxel(ev["x"], ev["y"], ev["t"], ev["p"], BINS, SENSOR, crop=CROP, mode="split", norm="minmax", check=False),
                "sort_only": None}
        keys = torch.randint(0, 11 * 289 * 385, (n,), dtype=torch.int32, device="cuda")
        legs["sort_only"] = lambda: torch.sort(keys, stable=True)
        diff = (legs["torch"]() - legs["hip"]()).abs().max().item()
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                times[k].append(timed(f, a.reps))
        with hip.launch_log() as log:
            legs["hip_nocheck"]()
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"N = {n}: torch composition {med['torch']:.3f} (min {min(times['torch']):.3f}, max {max(times['torch']):.3f}) | "
                     f"events_to_chunk {med['hip']:.3f} (min {min(times['hip']):.3f}, max {max(times['hip']):.3f}) | "
                     f"without the t-range read-back {med['hip_nocheck']:.3f} | torch stable sort alone {med['sort_only']:.3f} | "
                     f"speed-up {med['torch'] / med['hip']:.1f}x | max |torch - hip| {diff:.3g} (float atomics reorder the torch sums)")
        for name, wg, thr, lds, us in log.rows:
            lines.append(f"    {name.split('(')[0][-60:]:<60} {wg:>7} wg  {us:9.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
