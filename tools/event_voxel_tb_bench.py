#!/usr/bin/env python3
"""Time the MVSEC / MDR event front end on one MI355X, in one process: (i) the torch composition a user has without it - the
reference's EventSequenceToVoxelGrid_Pytorch steps restated on GPU tensors (float64 times, two index_add_ passes, per-list
normalisation; MDR_dataloader/loader_utils.py:470-575), centre crop, old | new, polarity split and min-max (harness.prepare_chunk) -
against (ii) harness.event_pairs_to_chunk (HIP), at the MVSEC shape: 2 lists of about 30 k events per sample, 10 bins per list,
260 x 346 -> 256 x 256, batch 1 and 4.  Device events around `reps` back-to-back calls after warm-up, the legs alternating, median of
`rounds`; the HIP leg's kernels come from the library's launch log, and the torch stable sort is timed alone.

    python tools/event_voxel_tb_bench.py [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdformerflow_amd import harness  # noqa: E402

SENSOR, CROP, BINS, EVENTS = (260, 346), (256, 256), 10, 30000


def synth_list(seed, n=EVENTS):
    r = np.random.default_rng(seed)
    t = 1.5e9 + np.sort(r.integers(0, 50000, n)) * 1e-6
    ev = {"ts": t, "x": r.integers(0, SENSOR[1], n).astype(np.int32), "y": r.integers(0, SENSOR[0], n).astype(np.int32),
          "p": r.integers(0, 2, n).astype(np.float32)}
    return {k: torch.from_numpy(v).cuda() for k, v in ev.items()}


def torch_voxel(ev, nb, H, W):
    """The reference class's steps on device tensors (index_add_ on the GPU is atomic: the sums are not reproducible)."""
    ts = ev["ts"] * 1e6
    ts = ts - ts[0]
    delta = ts[-1] - ts[0]
    delta = torch.where(delta == 0, torch.ones_like(delta), delta)
    ts = (nb - 1) * (ts - ts[0]) / delta
    xs, ys, pols = ev["x"].long(), ev["y"].long(), ev["p"].clone()
    pols[pols == 0] = -1
    tis = torch.floor(ts)
    tl, dts = tis.long(), (ts - tis).float()
    grid = torch.zeros(nb * H * W, dtype=torch.float32, device=ts.device)
    valid = (tis < nb) & (tis >= 0)
    grid.index_add_(0, (xs + ys * W + tl * W * H)[valid], (pols * (1.0 - dts))[valid])
    valid = (tis + 1 < nb) & (tis >= 0)
    grid.index_add_(0, (xs + ys * W + (tl + 1) * W * H)[valid], (pols * dts)[valid])
    grid = grid.view(nb, H, W)
    mask = torch.nonzero(grid, as_tuple=True)
    if mask[0].numel() > 0:
        mean, std = grid[mask].mean(), grid[mask].std()
        grid[mask] = (grid[mask] - mean) / std if std > 0 else grid[mask] - mean
    return grid


def torch_chunk(pairs):
    oy, ox = harness.center_crop_origin(SENSOR, CROP)
    vols = [torch.cat([torch_voxel(ev, BINS, *SENSOR) for ev in pair])[None, :, oy:oy + CROP[0], ox:ox + CROP[1]] for pair in pairs]
    chunk = harness.prepare_chunk(torch.cat(vols), "minmax", None, True)
    return chunk, chunk.sum(1).sum(1, keepdim=True).bool()


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
    from sdformerflow_amd import hip
    lines = [f"MVSEC / MDR event front end, 2 x {EVENTS} events per sample, 2 x {BINS} bins, {SENSOR} -> {CROP}, per-list normalisation, "
             f"minmax, event mask; ms per call, median of {a.rounds} rounds x {a.reps} calls ({torch.cuda.get_device_name(0)})"]
    for B in (1, 4):
        pairs = [(synth_list(10 * b + 1), synth_list(10 * b + 2)) for b in range(B)]
        keys = torch.randint(0, 2 * B * BINS * SENSOR[0] * SENSOR[1], (2 * B * EVENTS,), dtype=torch.int32, device="cuda")
        legs = {"torch": lambda: torch_chunk(pairs),
                "hip": lambda: harness.event_pairs_to_chunk(pairs, BINS, SENSOR, CROP, "minmax", None, want_event_mask=True),
                "sort_only": lambda: torch.sort(keys, stable=True)}
        (tc, tm), (hc, hm) = legs["torch"](), legs["hip"]()
        diff, mask_same = (tc - hc).abs().max().item(), bool(torch.equal(tm, hm != 0))
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                times[k].append(timed(f, a.reps))
        with hip.launch_log() as log:
            legs["hip"]()
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"batch {B}: torch composition {med['torch']:.3f} (min {min(times['torch']):.3f}, max {max(times['torch']):.3f}) | "
                     f"event_pairs_to_chunk {med['hip']:.3f} (min {min(times['hip']):.3f}, max {max(times['hip']):.3f}) | "
                     f"torch stable sort alone {med['sort_only']:.3f} | torch / hip {med['torch'] / med['hip']:.1f}x | "
                     f"max |torch - hip| {diff:.3g} (float atomics reorder the torch sums), event masks equal: {mask_same}")
        for name, wg, thr, lds, us in log.rows:
            kernel = re.search(r"\w+_kernel(<[^>]*>)?", name)
            lines.append(f"    {kernel.group(0) if kernel else name[-40:]:<28} {wg:>7} wg  {us:9.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
