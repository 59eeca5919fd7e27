#!/usr/bin/env python3
"""Generate tests/golden/augment.npz from the REAL reference transforms on the CPU (DSEC_dataloader/data_augmentation.py: Compose,
CenterCrop, RandomCrop, Random_horizontal_flip, Random_vertical_flip, Random_event_drop).

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_augment.py [path of the reference checkout]

The reference module imports torchvision for `transforms.functional.hflip` / `vflip`; where torchvision is absent a stand-in goes into
sys.modules whose hflip / vflip are `flip(-1)` / `flip(-2)` - what torchvision does to a tensor.  Only inputs (made here from a seed),
names, draws and the reference's outputs are stored.

Inputs: two items at (B, bins, Hs, Ws) = (2, 3, 11, 13) - a signed voxel with about 40 % zeros, a flow without zeros, a 0 / 1 mask -
all multiples of 1/4 below 16 in magnitude, so float16 stores them (and their gathered, negated or zeroed outputs, -0 included) exactly.
Chains: tests/augment_cases.chain_names() - every chain of the accepted form - at crop (8, 10).  Per chain the seeds (random.seed and
torch.manual_seed alike) are the first ones that show both outcomes of each of its coins; for the chains "RandomCrop" and
"RandomCrop,H,V,Drop" also both extreme rows and columns, and two more seeds that give the origins (0, 0) and (Hs - h, Ws - w).  A seed
at which `preserve_mosaicing_pattern` pushes the window out of the image (the reference then returns a clipped slice) is left out.
For a chain with a drop, the draws are replayed here under the same seed - the chain without its drop, then the coin, q and
`rand_like` on the tensor the drop saw - and stored as q (NaN: kept) and the uniform field u; the replay is checked against the
reference's output before anything is written.

Philox4x32-10 known answers: no file of the published vectors exists in this environment, so they are taken from an independent
implementation - ATen's `at::philox_engine` (torch/include/ATen/core/PhiloxRNGEngine.h), compiled here on the host into a small
program.  Stored as (seed, subsequence, offset) -> the block's four words; the engine's counter is (offset, subsequence)."""
import os
import random
import subprocess
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE", "/root/reference")
import augment_cases as A  # noqa: E402

KAT_IN = ((0, 0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), (0x299F31D0A4093822, 0x0370734413198A2E, 0x85A308D3243F6A88),
          (1234, 0, 5), (67280421310721, 3, 1 << 33), (7, 1 << 40, 0))
KAT_SRC = """
#include <ATen/core/PhiloxRNGEngine.h>
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  for (int i = 1; i + 2 < argc; i += 3) {
    at::philox_engine e(strtoull(argv[i], 0, 10), strtoull(argv[i + 1], 0, 10), strtoull(argv[i + 2], 0, 10));
    unsigned a = e(), b = e(), c = e(), d = e();
    printf("%u %u %u %u\\n", a, b, c, d);
  }
}
"""


def stand_ins():
    try:
        import torchvision.transforms  # noqa: F401
    except ImportError:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tr.functional = types.SimpleNamespace(hflip=lambda t: t.flip(-1), vflip=lambda t: t.flip(-2))
        tv.transforms = tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr


def make_item(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    B, bins, Hs, Ws = A.SHAPE
    vox = g.integers(-40, 41, (B, bins, Hs, Ws)) / 4.0
    vox = np.where(g.random(vox.shape) < 0.6, vox, 0.0)
    mag = g.integers(1, 60, (B, 2, Hs, Ws)) / 4.0
    flow = np.where(g.random(mag.shape) < 0.5, mag, -mag)
    mask = (g.random((B, 1, Hs, Ws)) < 0.7).astype(np.float32)
    return vox.astype(np.float32), flow.astype(np.float32), mask


def seeded(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def philox_known_answers():
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "kat.cpp"), os.path.join(tmp, "kat")
        open(src, "w").write(KAT_SRC)
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", inc, src, "-o", exe], check=True)
        out = subprocess.run([exe] + [str(v) for row in KAT_IN for v in row], check=True, capture_output=True, text=True).stdout
    return np.array([[int(w) for w in line.split()] for line in out.strip().split("\n")], dtype=np.uint32)


def main():
    stand_ins()
    sys.path.insert(0, REFERENCE)
    from DSEC_dataloader import data_augmentation as R
    items = [make_item(31), make_item(32)]
    out = {"shape": np.array(A.SHAPE), "crop": np.array(A.CROP), "chains": np.array(A.chain_names())}
    for k, (vox, flow, mask) in enumerate(items):
        out[f"in{k}_voxel"], out[f"in{k}_flow"], out[f"in{k}_mask"] = vox.astype(np.float16), flow.astype(np.float16), mask.astype(np.uint8)
        assert np.array_equal(out[f"in{k}_voxel"].astype(np.float32), vox) and np.array_equal(out[f"in{k}_flow"].astype(np.float32), flow)
    Hs, Ws = A.SHAPE[2:]
    top = (Hs - A.CROP[0], Ws - A.CROP[1])

    def origin_of(seed):
        random.seed(seed)
        return random.randint(0, top[0]), random.randint(0, top[1])
    corner = [next(s for s in range(1000) if origin_of(s) == o) for o in ((0, 0), top)]
    cases, seen_origins = [], set()
    marker = torch.arange(Hs * Ws, dtype=torch.float32).reshape(1, 1, Hs, Ws).expand(A.SHAPE[0], 1, Hs, Ws)

    def run(ci, name, parts, seed):
        """One case: the reference's outputs, and its draws - replayed under the same seed - as (origin, hflip, vflip, q, u); None
        where the mosaicing shift left the image (the reference returns a clipped slice)."""
        k = (ci + seed) % 2
        vox, flow, mask = (torch.from_numpy(a) for a in items[k])
        seeded(seed)
        ev, fl, mk = A.build_chain(R, name)((vox, flow, mask))
        if tuple(ev.shape[-2:]) != (A.CROP if "Crop" in name else (Hs, Ws)):
            return None
        head = ",".join(p for p in parts if p != "Drop")
        seeded(seed)
        ev0, fl0, mk0 = A.build_chain(R, head)((vox, flow, mask))
        q, u = np.float32("nan"), None
        if "Drop" in parts:
            if torch.rand(1).item() <= 0.5:
                qt = (0. - 0.6) * torch.rand(1) + 0.6
                ut = torch.rand_like(ev0)
                q, u = np.float32(qt.item()), ut.numpy().copy()
                ev0 = ev0 * (ut > qt)
        assert torch.equal(ev0, ev) and torch.equal(fl0, fl) and torch.equal(mk0, mk) and mk0.dtype == mk.dtype
        # the origin and the coins, read off a marker volume run through the same draws
        seeded(seed)
        mev = A.build_chain(R, head)((marker, flow, mask))[0]
        r0, c0 = divmod(int(mev[0, 0, 0, 0]), Ws)
        r1, c1 = divmod(int(mev[0, 0, -1, -1]), Ws)
        return k, (min(r0, r1), min(c0, c1)), c1 < c0, r1 < r0, q, u, ev, fl, mk

    for ci, name in enumerate(A.chain_names()):
        parts = [p for p in name.split(",") if p]
        random_crop = parts[:1] in (["RandomCrop"], ["RandomCropEven"])
        want = {(p, v) for p in parts if p in ("H", "V", "Drop") for v in (False, True)}
        full = name in ("RandomCrop", "RandomCrop,H,V,Drop")
        if full:
            want |= {("row", 0), ("row", top[0]), ("col", 0), ("col", top[1])}
        chosen = []
        # the first seeds that show something new; behind them, for the two full chains, the corner seeds whatever they show
        for seed, extra in [(s, False) for s in range(200)] + [(s, True) for s in corner if full]:
            if seed in chosen or (chosen and not want and not extra):
                continue
            rec = run(ci, name, parts, seed)
            if rec is None:
                continue
            k, origin, hflip, vflip, q, u, ev, fl, mk = rec
            got = {("H", hflip), ("V", vflip), ("Drop", u is not None), ("row", origin[0]), ("col", origin[1])}
            if want and not extra and not (got & want):
                continue
            want -= got
            chosen.append(seed)
            if random_crop:
                seen_origins.add(origin)
            tag = f"c{ci}_s{seed}"
            cases.append((ci, seed, k, origin[0], origin[1], int(hflip), int(vflip)))
            out[tag + "_events"], out[tag + "_flow"] = ev.numpy().astype(np.float16), fl.numpy().astype(np.float16)
            assert np.array_equal(out[tag + "_events"].astype(np.float32).view(np.int32), ev.numpy().view(np.int32))
            assert np.array_equal(out[tag + "_flow"].astype(np.float32).view(np.int32), fl.numpy().view(np.int32))
            out[tag + "_mask"] = mk.numpy().astype(np.uint8)
            out[tag + "_mask_is_bool"] = np.array(mk.dtype == torch.bool)
            out[tag + "_q"] = np.array(q, dtype=np.float32)
            if u is not None:
                out[tag + "_u"] = u
        assert not want and chosen, (name, want)
    assert (0, 0) in seen_origins and top in seen_origins
    # (chain, seed, input, origin row, origin column, hflip, vflip) of every case
    out["cases"] = np.array(cases, dtype=np.int64)
    out["philox_kat_in"] = np.array(KAT_IN, dtype=np.uint64)
    out["philox_kat_out"] = philox_known_answers()
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
