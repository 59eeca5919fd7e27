#!/usr/bin/env python3
"""Generate tests/golden/mdr_augment.npz from the REAL reference class MDR_dataloader.loader_utils.DenseSparseAugmentor on the CPU,
and the item's `valid` from the real MDREventFlow.__getitem__ (MDR_dataloader/MDR.py:218-241) around it.

Needs a checkout of the reference, which the tests themselves never read:

    python tests/golden/make_golden_mdr_augment.py <path of the reference checkout>      (or SDF_REFERENCE in the environment)

loader_utils.py and MDR.py import cv2, torchvision, h5py and others at their top; where they are absent, stand-ins go into sys.modules.
cv2 is absent, and DenseSparseAugmentor calls cv2.resize: the stand-in's `resize` is this package's `resize_linear`, the restatement
of cv2.resize(INTER_LINEAR).  The consequence: the draws and their order, the clip of the scales, the output size the reference asks
for (fx, fy; checked here against the image the stand-in returns), the flips, the crop, the float64 flow scaling and the `valid`
expression are the reference's own code - but the interpolated values are this package's, not a real cv2 build's.

Inputs (tests/mdr_augment_cases.py fixture_inputs, from a seed): frames 21 x 25, 3 channels per volume, multiples of 1/4 with about
40 % zeros, a flow with a few exact zeros, one inf and one NaN.  Parameters: crop (8, 10), min_scale -0.3, max_scale 0.5, do_flip True.
Seeds: counted up from 0, a seed is kept when it shows a property no kept seed has shown - resized / not, stretched / not, each flip
both ways, a scale clipped from below, a resized axis below 1 and one above 1, origin 0 and the largest in each axis - until all are
shown.  Stored per seed: the inputs' index, the parameter record (this package's `sample` under the same seed, checked here against
what the reference did: the scales it passed to cv2.resize, its outputs, and the generator's state behind it), the next
np.random.rand() after the call, the five outputs as the reference returns them (the flow float64 unless nothing touched it), and
the item's float flow and `valid`."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ["SDF_REFERENCE"]

import mdr_augment_cases as M  # noqa: E402
from sdformerflow_amd.MDR_dataloader import loader_utils as L  # noqa: E402

RESIZE_CALLS = []


def fake_resize(img, dsize, fx=None, fy=None, interpolation=None):
    assert dsize is None and interpolation == "linear"
    out = L.resize_linear(img, fx, fy)
    RESIZE_CALLS.append((float(fx), float(fy), out.shape[:2]))
    return out


def stand_ins():
    for name in ("cv2", "torchvision", "torchvision.transforms", "PIL", "PIL.Image", "h5py", "pandas", "matplotlib", "matplotlib.pyplot",
                 "matplotlib.colors"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.setNumThreads = lambda *a: None
            m.ocl = types.SimpleNamespace(setUseOpenCL=lambda *a: None)
            m.ColorJitter = lambda **kw: None
            m.Image = m.RandomCrop = m.pyplot = m.colors = object
            sys.modules[name] = m
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], m)
    cv2 = sys.modules["cv2"]
    if not hasattr(cv2, "resize"):
        cv2.resize, cv2.INTER_LINEAR = fake_resize, "linear"
    return cv2.resize is fake_resize


def properties(p, stretched, floor):
    top = (p.size[0] - M.CROP[0] - 1, p.size[1] - M.CROP[1] - 1)           # randint's upper end is exclusive
    got = {("resized", p.resized), ("stretched", stretched), ("hflip", p.hflip), ("vflip", p.vflip)}
    if p.scale_x == floor or p.scale_y == floor:
        got.add("clipped")
    if p.resized:
        got |= {"below 1" for s in (p.scale_x, p.scale_y) if s < 1} | {"above 1" for s in (p.scale_x, p.scale_y) if s > 1}
    got |= {f"y0 {'0' if p.y0 == 0 else 'top'}" for _ in (1,) if p.y0 in (0, top[0])}
    got |= {f"x0 {'0' if p.x0 == 0 else 'top'}" for _ in (1,) if p.x0 in (0, top[1])}
    return got


WANTED = {("resized", True), ("resized", False), ("stretched", True), ("stretched", False), ("hflip", True), ("hflip", False),
          ("vflip", True), ("vflip", False), "clipped", "below 1", "above 1", "y0 0", "y0 top", "x0 0", "x0 top"}


def main():
    ours = stand_ins()
    sys.path.insert(0, REFERENCE)
    from MDR_dataloader.loader_utils import DenseSparseAugmentor
    from MDR_dataloader.MDR import MDREventFlow
    ref = DenseSparseAugmentor(list(M.CROP), min_scale=M.MIN_SCALE, max_scale=M.MAX_SCALE, do_flip=True)
    mine = L.DenseSparseAugmentor(list(M.CROP), min_scale=M.MIN_SCALE, max_scale=M.MAX_SCALE, do_flip=True)
    for k in ("spatial_aug_prob", "stretch_prob", "max_stretch", "h_flip_prob", "v_flip_prob", "do_flip", "crop_size", "min_scale", "max_scale"):
        assert getattr(ref, k) == getattr(mine, k), k
    floor = max((M.CROP[0] + 8) / M.FRAME[0], (M.CROP[1] + 8) / M.FRAME[1])
    item = MDREventFlow.__new__(MDREventFlow)                               # (no files: the sample is handed in)
    item.type, item.pol, item.dense_augmentor, item.names = "train", True, ref, [0]
    out = {"frame": np.array(M.FRAME), "crop": np.array(M.CROP), "scales": np.array([M.MIN_SCALE, M.MAX_SCALE]),
           "cv2_is_restated": np.array(ours)}
    shown, seeds, rows = set(), [], []
    seed = -1
    while shown != WANTED:
        seed += 1
        assert seed < 2000, WANTED - shown
        k = seed % 2
        vols, flow = M.fixture_inputs(k)
        np.random.seed(seed)
        p = mine.sample(M.FRAME)
        np.random.seed(seed)
        np.random.uniform()
        stretched = bool(np.random.rand() < ref.stretch_prob)
        new = properties(p, stretched, floor) & WANTED
        if new <= shown:
            continue
        shown |= new
        # the reference, under the same seed
        del RESIZE_CALLS[:]
        np.random.seed(seed)
        got = ref(*[v.copy() for v in vols], flow.copy())
        after = np.random.rand()
        if ours:
            assert len(RESIZE_CALLS) == (5 if p.resized else 0)
            assert all(c == (p.scale_x, p.scale_y, tuple(p.size)) for c in RESIZE_CALLS), (seed, p, RESIZE_CALLS)
        np.random.seed(seed)
        again = mine(*[v.copy() for v in vols], flow.copy())
        assert after == np.random.rand()
        for a, b in zip(got, again):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (seed, p)
        # the item around it: .float() of everything and `valid`
        item.get_sample = lambda idx: {"event_volume_old": torch.from_numpy(vols[0].copy()).permute(2, 0, 1),
                                       "event_volume_new": torch.from_numpy(vols[1].copy()).permute(2, 0, 1),
                                       "d_event_volume_old": torch.from_numpy(vols[2].copy()).permute(2, 0, 1),
                                       "d_event_volume_new": torch.from_numpy(vols[3].copy()).permute(2, 0, 1),
                                       "flow": torch.from_numpy(flow.copy()).permute(2, 0, 1)}
        np.random.seed(seed)
        with np.errstate(invalid="ignore"):
            sample = item[0]
        assert torch.equal(sample["d_event_volume_new"], torch.from_numpy(got[3]).permute(2, 0, 1))
        tag = f"s{seed}"
        for name, a in zip(("img1", "img2", "dimg1", "dimg2", "flow"), got):
            out[f"{tag}_{name}"] = a
        out[f"{tag}_item_flow"], out[f"{tag}_valid"] = sample["flow"].numpy(), sample["valid"].numpy()
        out[f"{tag}_after"] = np.array(after)
        seeds.append((seed, k))
        rows.append(M.record_of(p))
        print(seed, k, p, "stretched" if stretched else "", sorted(map(str, new)))
    out["seeds"], out["records"] = np.array(seeds), np.array(rows)
    for k in (0, 1):
        vols, flow = M.fixture_inputs(k)
        out[f"in{k}_vols"], out[f"in{k}_flow"] = np.stack(vols), flow
    path = os.path.join(HERE, "mdr_augment.npz")
    np.savez_compressed(path, **out)
    print(len(seeds), "seeds; bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
