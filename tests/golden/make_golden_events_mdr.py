#!/usr/bin/env python3
"""Generate tests/golden/events_voxel_mdr.npz from the REAL reference classes on the CPU: EventSequence(..., timestamp_multiplier=1e6,
convert_to_relative=True) and EventSequenceToVoxelGrid_Pytorch(gpu=False) (MDR_dataloader/loader_utils.py:344-389, 421-577) on small
seeded event lists, and for one pair the tensor steps of the evaluation loop (eval_MV_flow_SNN.py:162-219) applied to the reference's
volumes.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_events_mdr.py [path of the reference checkout]

loader_utils.py imports cv2, torchvision and PIL at its top for its augmentors; where they are absent, empty stand-ins go into
sys.modules (the two classes use none of them).  Only inputs (the event lists, made here from a seed) and the reference's outputs are
stored.  The reference cannot take an empty list (it indexes the last event); list "d" stores the zero grids this package documents.

Lists, all (N, 4) float64 [ts seconds, x, y, p] in time order:
  a, b  5 x 36 x 44, epoch stamps near 1.5e9 s on a microsecond grid (about three events per tick), five events at the last stamp, two
        hot pixels with 600 / 300 (a) and 472 / 300 (b) events inside one bin; p is 0 / 1 in a and -1 / +1 in b.  (a, b) is the stored pair.
  c     one distinct time stamp;  d  empty;  e  one event;  f  10 x 30 x 40, p -1 / +1, relative stamps."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE", "/root/reference")
# name, (nb, H, W), events, seed, polarity values, first stamp (s)
CASES = (("a", (5, 36, 44), 4000, 21, (0, 1), 1.5e9), ("b", (5, 36, 44), 3000, 22, (-1, 1), 1.5e9 + 0.05),
         ("c", (5, 36, 44), 50, 23, (-1, 1), 1.5e9), ("d", (5, 36, 44), 0, 24, (0, 1), 0.0), ("e", (5, 36, 44), 1, 25, (0, 1), 1.5e9),
         ("f", (10, 30, 40), 2500, 26, (-1, 1), 0.0))


def stand_ins():
    for name in ("cv2", "torchvision", "torchvision.transforms", "PIL", "PIL.Image"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.setNumThreads = lambda *a: None
            m.ocl = types.SimpleNamespace(setUseOpenCL=lambda *a: None)
            m.ColorJitter = m.Image = object
            sys.modules[name] = m
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], m)


def make_events(size, n, seed, pols, t0, single_time=False):
    """The fixture's event list, (n, 4) float64 [ts seconds, x, y, p], time-ordered."""
    nb, H, W = size
    r = np.random.default_rng(seed)
    x = r.integers(0, W, n).astype(np.float64)
    y = r.integers(0, H, n).astype(np.float64)
    ticks = np.sort(r.integers(0, max(n // 3, 1), n)).astype(np.float64)
    if n >= 5:
        ticks[-5:] = ticks[-1]                                               # tis = nb - 1: the left pass only
    if single_time:
        ticks[:] = 7.0
    if n >= 2000:                                                            # hot pixels: 600 / 300 events inside one bin each
        span = ticks[-1] / (nb - 1)
        first = np.flatnonzero((ticks > 0.05 * span) & (ticks < 0.95 * span))
        second = np.flatnonzero((ticks > 1.05 * span) & (ticks < 1.95 * span))
        hot1 = r.choice(first, min(600, int(0.7 * first.size)), replace=False)             # (fewer where a bin holds fewer: list f)
        hot2 = r.choice(second, min(300, int(0.7 * second.size)), replace=False)
        x[hot1], y[hot1] = 7.0, 9.0
        x[hot2], y[hot2] = 3.0, 4.0
    t = t0 + ticks * 1e-6
    p = r.choice(np.array(pols, dtype=np.float64), n)
    return np.stack([t, x, y, p], axis=1)


def loop_chunk(old, new):
    """eval_MV_flow_SNN.py:162-219 on one sample: num_chunks 2, encoding voxel, loader.polarity true, norm_input minmax, spike_th
    None, metrics.mask_events true."""
    chunk = torch.cat((old[None], new[None]), dim=1)
    neg = torch.nn.functional.relu(-chunk)
    pos = torch.nn.functional.relu(chunk)
    chunk = torch.cat((torch.unsqueeze(pos, dim=2), torch.unsqueeze(neg, dim=2)), dim=2)
    lo, hi = torch.min(chunk[chunk != 0]), torch.max(chunk[chunk != 0])
    if not lo == hi:
        chunk[chunk != 0] = (chunk[chunk != 0] - lo) / (hi - lo)
    event_mask = torch.sum(torch.sum(chunk, dim=1), dim=1, keepdim=True).bool()
    return chunk, event_mask


def main():
    stand_ins()
    sys.path.insert(0, REFERENCE)
    from MDR_dataloader.loader_utils import EventSequence, EventSequenceToVoxelGrid_Pytorch
    out, norm = {}, {}
    for name, size, n, seed, pols, t0 in CASES:
        nb, H, W = size
        ev = make_events(size, n, seed, pols, t0, single_time=(name == "c"))
        out[name + "_size"] = np.array(size, dtype=np.int32)
        out[name + "_events"] = ev
        for key, kw in (("raw", dict(normalize=False)), ("norm", dict(normalize=True)), ("pol", dict(normalize=False, pol=False)),
                        ("poln", dict(normalize=True, pol=False))):
            if n == 0:
                grid = torch.zeros((nb, H, W) if "pol" not in key else (nb, 2, H, W))
            else:
                seq = EventSequence(None, {"height": H, "width": W}, features=ev.copy(), timestamp_multiplier=1e6, convert_to_relative=True)
                grid = EventSequenceToVoxelGrid_Pytorch(nb, gpu=False, forkserver=False, **kw)(seq)
            out[f"{name}_{key}"] = grid.contiguous().numpy().astype(np.float32)
        norm[name] = torch.from_numpy(out[name + "_norm"])
        g = out[name + "_raw"]
        print(name, size, n, "events: non-zero cells", int((g != 0).sum()), "min", g.min(), "max", g.max(), "normalised max",
              np.abs(out[name + "_norm"]).max())
    chunk, mask = loop_chunk(norm["a"], norm["b"])
    out["ab_chunk"], out["ab_event_mask"] = chunk.numpy(), mask.numpy()
    np.savez_compressed(os.path.join(HERE, "events_voxel_mdr.npz"), **out)
    print("bytes", os.path.getsize(os.path.join(HERE, "events_voxel_mdr.npz")))


if __name__ == "__main__":
    main()
