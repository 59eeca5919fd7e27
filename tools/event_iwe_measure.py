#!/usr/bin/env python3
"""Time the image of warped events and the Flow Warp Loss on one MI355X, in one process, at the DSEC shape: 480 x 640, one list of
N = 1e6 and 4e6 events (tests/test_event_voxel_gpu.synth_events' recipe), a smooth flow of a few pixels.  Legs: hip.event_iwe in each
mode (without the t-range read-back), the torch stable sort alone (the sort's share), hip.iwe_stats, the whole FWL of a sample
(loss.flow_warp.FWL: two nearest warps, two statistics) and a torch composition of the same arithmetic - one
index_put_(accumulate=True) pass per corner, float atomics, no stated order of a cell's sum (the run reports whether three repeats
of either side were bit-equal, and the largest difference between the two).  Device events around `reps`
back-to-back calls after warm-up, the legs alternating, median of `rounds`; the HIP legs are also split into their kernels from the
library's launch log.

    python tools/event_iwe_measure.py [--rounds 7] [--reps 10] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sdformerflow_amd import hip  # noqa: E402
from sdformerflow_amd.loss.flow_warp import FWL  # noqa: E402

SENSOR = (480, 640)


def torch_iwe(ev, flow, scale=1.0, t_ref=1.0, mode="bilinear"):
    """csrc/event_iwe.hip's arithmetic as torch operations on the whole sensor, window (0, 1): index_put_ with float atomics."""
    H, W = flow.shape[-2:]
    x, y, t, p = ev["x"], ev["y"], ev["t"], ev["p"]
    tau = (t - t[0]) / (t[-1] - t[0])
    fx, fy = torch.floor(x + 0.5), torch.floor(y + 0.5)
    keep = (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    xi, yi = torch.where(keep, fx, 0).long(), torch.where(keep, fy, 0).long()
    u, v = scale * flow[0, 0, yi, xi], scale * flow[0, 1, yi, xi]
    keep &= torch.isfinite(u) & torch.isfinite(v)
    d = t_ref - tau
    xw, yw = x + d * u, y + d * v
    ch = torch.where(p > 0, 0, 1)
    out = torch.zeros(2 * H * W, dtype=torch.float32, device=x.device)
    if mode == "nearest":
        corners = [(torch.round(xw), torch.round(yw))]
    else:
        x0, y0 = torch.floor(xw), torch.floor(yw)
        corners = [(x0 + dx, y0 + dy) for dx in (0, 1) for dy in (0, 1)]
    for xc, yc in corners:
        ok = keep & (xc >= 0) & (xc < W) & (yc >= 0) & (yc < H)
        wgt = torch.ones_like(xw) if mode == "nearest" else (1 - (xc - xw).abs()) * (1 - (yc - yw).abs())
        index = (ch * H + torch.where(ok, yc, 0).long()) * W + torch.where(ok, xc, 0).long()
        out.index_put_((index[ok],), wgt[ok], accumulate=True)
    return out.view(1, 2, H, W)


def torch_fwl(ev, flow, scale):
    var = lambda img: img.sum(1).double().var()
    return var(torch_iwe(ev, flow, scale, mode="nearest")) / var(torch_iwe(ev, flow, 0.0, mode="nearest"))


def short(name):
    """A kernel's name as the launch log has it, without its return type, namespace and parameter list."""
    name = re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", name))
    return re.sub(r"\(.*$", "", name)[-60:]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def smooth_flow(H, W, seed=9):
    r = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    a = r.uniform(-8, 8, 6)
    return np.stack([a[0] + a[1] * xx + a[2] * yy, a[3] + a[4] * xx + a[5] * yy]).astype(np.float32)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from test_event_voxel_gpu import synth_events
    flow = torch.from_numpy(smooth_flow(*SENSOR)).cuda()
    lines = [f"image of warped events and FWL, {SENSOR}, one list; ms per call, median (min .. max) of {a.rounds} rounds x {a.reps} "
             f"calls ({torch.cuda.get_device_name(0)})"]
    for n in (1000000, 4000000):
        ev = {k: torch.from_numpy(v).cuda() for k, v in synth_events(n, seed=3).items()}
        iwe = lambda mode: hip.event_iwe(ev["x"], ev["y"], ev["t"], ev["p"], flow, SENSOR, mode=mode, check=False)
        near = iwe("nearest")
        keys = torch.randint(0, 2 * 481 * 641, (n,), dtype=torch.int32, device="cuda")
        legs = {"hip bilinear": lambda: iwe("bilinear"), "hip nearest": lambda: iwe("nearest"),
                "torch stable sort alone": lambda: torch.sort(keys, stable=True), "hip.iwe_stats": lambda: hip.iwe_stats(near),
                "FWL (hip)": lambda: FWL(flow, ev, SENSOR, None, 1.0)(), "torch bilinear": lambda: torch_iwe(ev, flow),
                "torch nearest": lambda: torch_iwe(ev, flow, mode="nearest"), "FWL (torch)": lambda: torch_fwl(ev, flow, 1.0)}
        diff = {m: (torch_iwe(ev, flow, mode=m) - iwe(m)).abs().max().item() for m in ("bilinear", "nearest")}
        same = all(torch.equal(iwe("bilinear"), iwe("bilinear")) for _ in range(3))
        torch_same = all(torch.equal(torch_iwe(ev, flow), torch_iwe(ev, flow)) for _ in range(3))
        fwl_hip, fwl_torch = legs["FWL (hip)"]()[0].item(), legs["FWL (torch)"]().item()
        for f in legs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, f in legs.items():
                times[k].append(timed(f, a.reps))
        lines.append(f"N = {n}: max |torch - hip| bilinear {diff['bilinear']:.3g}, nearest {diff['nearest']:.3g}; hip runs bit-equal: {same}; "
                     f"torch runs bit-equal: {torch_same}; FWL hip {fwl_hip:.6f}, torch {fwl_torch:.6f}")
        for k, v in times.items():
            lines.append(f"    {k:<26} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})")
        for mode in ("bilinear", "nearest"):
            with hip.launch_log() as log:
                iwe(mode)
            lines.append(f"    kernels of hip {mode} (the stable sort between keys and runs is torch's):")
            for name, wg, thr, lds, us in log.rows:
                lines.append(f"        {short(name):<60} {wg:>7} wg  {us:9.1f} us")
        with hip.launch_log() as log:
            hip.iwe_stats(near)
        for name, wg, thr, lds, us in log.rows:
            lines.append(f"        {short(name):<60} {wg:>7} wg  {us:9.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
