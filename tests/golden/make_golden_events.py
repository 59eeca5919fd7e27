#!/usr/bin/env python3
"""Generate tests/golden/events_voxel.npz from the REAL reference class on the CPU: VoxelGrid.convert_CHW and
convert_CHW_polarities (DSEC_dataloader/event_representations.py:241-313) on small seeded event lists.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_events.py [path of the reference checkout]

The reference module imports numba, h5py, hdf5plugin and tqdm at its top for its file readers; where they are absent, empty
stand-ins go into sys.modules (VoxelGrid uses none of them).  Only inputs (the event lists, made here from a seed) and the
reference's outputs are stored.

Each list holds, in time order: fractional and integer coordinates, x, y in (-1, 0) (truncation makes their base cell 0 and some
weights negative), x >= W - 1 and y >= H - 1 (the upper corners fall outside), coordinates fully outside, two hot pixels with
hundreds of events on one cell, many equal timestamps, both polarities, and several events at the last time (t_norm = C - 1)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE", "/root/reference")
CASES = (("a", (5, 24, 32), 3000, 11), ("b", (10, 30, 40), 4000, 12))       # name, (C, H, W), events, seed


def stand_ins():
    for name in ("numba", "h5py", "hdf5plugin", "tqdm"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.jit = lambda *a, **k: (lambda f: f)
            m.File = object
            m.PLUGINS_PATH = ""
            sys.modules[name] = m


def make_events(C, H, W, n, seed):
    """The fixture's event list (x, y, t, p fp32, time-ordered)."""
    r = np.random.default_rng(seed)
    x = r.uniform(-1.5, W + 0.5, n)
    y = r.uniform(-1.5, H + 0.5, n)
    k = n // 8
    x[:k], y[:k] = np.floor(x[:k]), np.floor(y[:k])                          # integer pixels (sensor coordinates that need no rectification)
    x[k:k + 40], y[k + 40:k + 80] = r.uniform(-0.999, -0.001, 40), r.uniform(-0.999, -0.001, 40)
    x[k + 80:k + 120], y[k + 120:k + 160] = r.uniform(W - 1, W - 0.01, 40), r.uniform(H - 1, H - 0.01, 40)
    x[k + 160:k + 180], y[k + 180:k + 200] = -5.25, H + 10.5                 # fully outside
    x[k + 200:k + 210], y[k + 200:k + 210] = -1.0, -1.0                      # base cell -1: weight 0 on cell 0
    hot = k + 210 + r.permutation(n - k - 210)                               # (none of the special events above)
    x[hot[:600]], y[hot[:600]] = 7.25, 9.5                                   # hot pixels: one fractional, one on the pixel centre
    x[hot[600:900]], y[hot[600:900]] = 3.0, 4.0
    t = np.sort(r.integers(0, n // 3, n)).astype(np.float64) + 1.0e5         # microsecond ticks, about three events per tick
    t[-5:] = t[-1]
    p = r.integers(0, 2, n)
    return {"x": x.astype(np.float32), "y": y.astype(np.float32), "t": t.astype(np.float32), "p": p.astype(np.float32)}


def main():
    stand_ins()
    sys.path.insert(0, REFERENCE)
    from DSEC_dataloader.event_representations import VoxelGrid
    out = {}
    for name, size, n, seed in CASES:
        ev = make_events(*size, n, seed)
        tev = {k: torch.from_numpy(v) for k, v in ev.items()}
        out[name + "_size"] = np.array(size, dtype=np.int32)
        for k, v in ev.items():
            out[f"{name}_{k}"] = v
        out[name + "_chw"] = VoxelGrid(size).convert_CHW(tev).numpy()
        out[name + "_pol"] = VoxelGrid(size).convert_CHW_polarities(tev).numpy()
        g = out[name + "_chw"]
        print(name, size, n, "events: grid nonzero", int((g != 0).sum()), "min", g.min(), "max", g.max(), "pol", out[name + "_pol"].shape)
    np.savez_compressed(os.path.join(HERE, "events_voxel.npz"), **out)


if __name__ == "__main__":
    main()
