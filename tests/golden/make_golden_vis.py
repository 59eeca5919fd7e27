#!/usr/bin/env python3
"""Generate tests/golden/visualization.npz from the REAL reference class on the CPU: Visualization_DSEC.flow_to_image and
events_to_image (utils/visualization.py:257-341, numpy + matplotlib) and the uint16 array its store() hands to imageio for
`flow_test` (:198-207), on small seeded inputs.

Run in the build container only (needs the reference checkout and matplotlib; neither exists on the GPU box):

    python tests/golden/make_golden_vis.py [path of the reference checkout]

utils/visualization.py imports cv2, imageio and pandas at its top; where they are absent, empty stand-ins go into sys.modules, with an
`imwrite` that keeps the array store() hands over (the two static methods use none of them - which is also why the BYTES cv2.imwrite
makes of the event image are not in the fixture: only the float image is).  Only inputs and the reference's outputs are stored.

Flow fields (fp32, `flow/<name>` (2, H, W) -> `flow_img/<name>` (H, W, 3) u8, `sub/<name>` (H, W, 3) u16):
  rand16x24, rand5x7  normal flows of a few pixels
  const               one vector everywhere: magnitude range 0, the value stays undivided (0: black)
  zero                all zero
  hue_edges           fx < 0 with fy = +0.0 / -0.0 (hue exactly 1.0 and 0.0) among ordinary pixels, and the four axis directions
Event counts (fp32, `events/<name>` (2, h, w) -> `events_img/<name>` (h, w, 3) float64, the reference's image (0, pos', neg')):
  poisson             dense Poisson counts of both polarities
  zero                no event at all
  sparse              under 1 % of the pixels non-zero: both percentiles 0, so the un-normalised branch (clip only)
  posmin_eq_max       constant positive counts 3, negatives of 1 or 2 on a sixth of the pixels (pos_min == max == 3: the positive polarity is only
                      clipped, the negative one divided by 3)"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE", "/root/reference")

WRITTEN = {}                                                      # file name -> the array the reference handed to its image writer


def stand_ins():
    """cv2 / imageio / pandas stand-ins where they are absent; their `imwrite` keeps what store() hands over instead of writing it."""
    def keep(filename, img, **kw):
        WRITTEN[filename] = np.array(img)
    for name in ("cv2", "imageio", "pandas"):
        try:
            m = __import__(name)
        except ImportError:
            m = sys.modules[name] = types.ModuleType(name)
        m.imwrite, m.waitKey = keep, lambda *a: None


def flow_fields():
    r = np.random.default_rng(31)
    f = {"rand16x24": (r.standard_normal((2, 16, 24)) * 6).astype(np.float32),
         "rand5x7": (r.standard_normal((2, 5, 7)) * 0.7).astype(np.float32),
         "const": np.broadcast_to(np.array([1.5, -2.25], np.float32)[:, None, None], (2, 6, 9)).copy(),
         "zero": np.zeros((2, 4, 6), np.float32)}
    e = (r.standard_normal((2, 8, 10)) * 3).astype(np.float32)
    e[0, 0, :5] = -np.abs(e[0, 0, :5]) - 0.5
    e[1, 0, :5] = 0.0
    e[0, 1, :5] = -np.abs(e[0, 1, :5]) - 0.5
    e[1, 1, :5] = -0.0
    e[:, 2, 0], e[:, 2, 1], e[:, 2, 2], e[:, 2, 3] = (2.0, 0.0), (0.0, 2.0), (-2.0, 0.0), (0.0, -2.0)
    f["hue_edges"] = e
    return f


def event_counts():
    r = np.random.default_rng(32)
    c = {"poisson": r.poisson(2.0, (2, 18, 26)).astype(np.float32),
         "zero": np.zeros((2, 6, 8), np.float32)}
    s = np.zeros((2, 30, 40), np.float32)
    for p in range(2):
        at = r.choice(30 * 40, 9, replace=False)                 # 9 of 1200 pixels: 0.75 %
        s[p].reshape(-1)[at] = r.uniform(0.2, 2.5, 9).astype(np.float32)
    c["sparse"] = s
    q = np.zeros((2, 12, 15), np.float32)
    q[0] = 3.0
    q[1].reshape(-1)[r.choice(180, 30, replace=False)] = r.integers(1, 3, 30).astype(np.float32)
    c["posmin_eq_max"] = q
    return c


def main():
    stand_ins()
    sys.path.insert(0, REFERENCE)
    from utils.visualization import Visualization_DSEC as V
    tmp = tempfile.mkdtemp()
    vis = V({"vis": {"px": 400}}, eval_id=0, path_results=tmp + "/")
    out = {}
    for name, f in flow_fields().items():
        out[f"flow/{name}"] = f
        hwc = f.transpose(1, 2, 0)                                # store()'s layout: (H, W, 2) from the (1, 2, H, W) tensor
        img = V.flow_to_image(hwc[:, :, 0], hwc[:, :, 1])
        assert img.dtype == np.uint8 and img.shape == f.shape[1:] + (3,)
        out[f"flow_img/{name}"] = img
        # the benchmark encoding: what store() hands to imageio for `flow_test` (its event image goes to the stand-in too, unused)
        vis.store(torch.zeros(1, 2, *f.shape[1:]), None, None, None, name, flow_test=torch.from_numpy(f)[None], idx=7)
        sub = WRITTEN[os.path.join(tmp, "results", "eval_0", "flow_test", name, "000007.png")]
        assert sub.dtype == np.uint16 and sub.shape == f.shape[1:] + (3,)
        out[f"sub/{name}"] = sub
    for name, c in event_counts().items():
        out[f"events/{name}"] = c
        img = V.events_to_image(c.transpose(1, 2, 0).copy())
        assert img.dtype == np.float64 and img.shape == c.shape[1:] + (3,)
        out[f"events_img/{name}"] = img
    path = os.path.join(HERE, "visualization.npz")
    np.savez_compressed(path, **out)
    shutil.rmtree(tmp)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
