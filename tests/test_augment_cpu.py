"""The training front end without a GPU: `Compose.sample` and the torch transforms of sdformerflow_amd.DSEC_dataloader.data_augmentation
against the reference's own outputs (tests/golden/augment.npz, made by tests/golden/make_golden_augment.py from the reference's classes)
through the numpy restatement of the kernel (tests/augment_cases.py); the restatement's Philox4x32-10; and the new entry points in the
header, in the binding's signature table, and their argument checks (refused before any launch)."""
import ctypes as C
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_cases as A  # noqa: E402

NEW = ("sdf_augment_chunk_workspace_bytes", "sdf_augment_chunk_fwd")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))
    assert tuple(z["shape"]) == A.SHAPE and tuple(z["crop"]) == A.CROP and list(z["chains"]) == A.chain_names()
    return z


def cases(z):
    """(chain name, seed, inputs (voxel, flow, mask) fp32, recorded (origin, flags), q or None, u or None, reference outputs)."""
    for ci, seed, k, oy, ox, hf, vf in z["cases"].tolist():
        tag = f"c{ci}_s{seed}"
        q = float(z[tag + "_q"])
        inputs = tuple(z[f"in{k}_{n}"].astype(np.float32) for n in ("voxel", "flow", "mask"))
        want = (z[tag + "_events"].astype(np.float32), z[tag + "_flow"].astype(np.float32), z[tag + "_mask"], bool(z[tag + "_mask_is_bool"]))
        yield A.chain_names()[ci], seed, inputs, ((oy, ox), hf | vf << 1), (None if math.isnan(q) else q), (z[tag + "_u"] if tag + "_u" in z else None), want


def seeded(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def test_fixture_covers_every_chain_coin_and_corner(golden):
    rows = list(cases(golden))
    names = [r[0] for r in rows]
    assert set(names) == set(A.chain_names()) and len(A.chain_names()) == 34
    top = (A.SHAPE[2] - A.CROP[0], A.SHAPE[3] - A.CROP[1])
    origins = {r[3][0] for r in rows if r[0].startswith("RandomCrop")}
    assert (0, 0) in origins and top in origins
    for name in A.chain_names():
        mine = [r for r in rows if r[0] == name]
        parts = name.split(",")
        if "H" in parts:
            assert {r[3][1] & 1 for r in mine} == {0, 1}, name
        if "V" in parts:
            assert {r[3][1] >> 1 for r in mine} == {0, 1}, name
        if "Drop" in parts:
            assert {r[4] is None for r in mine} == {False, True}, name
            assert all((r[4] is None) == (r[5] is None) and (r[4] is None or 0.0 <= r[4] <= 0.6) for r in mine)


def test_sample_and_restatement_equal_the_reference(golden):
    """`Compose.sample` under the fixture's seeds draws the reference's parameters (the recorded origin and coins, the drop's q), and
    the numpy restatement of the kernel's gather, fed with them and the recorded uniform field, gives the reference's outputs bit for
    bit: the draw order, the gather and its sign rule, and the drop as a multiplication (-0 where a negative event is dropped)."""
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    B = A.SHAPE[0]
    n = 0
    for name, seed, (vox, flow, mask), (origin, flags), q, u, (ev, fl, mk, _) in cases(golden):
        seeded(seed)
        p = A.build_chain(D, name).sample(vox.shape)
        assert (tuple(p.origin), p.flags) == (origin, flags), (name, seed, p)
        assert tuple(p.crop) == (A.CROP if "Crop" in name else A.SHAPE[2:])
        assert (p.drop_q is None) == (q is None) and (q is None or np.float32(p.drop_q) == np.float32(q)), (name, seed, p.drop_q, q)
        origins, flips, qs = p.per_sample(B)
        got = A.gather(vox, flow, mask, tuple(p.crop), origins, flips, qs, drop_u=u)
        assert np.array_equal(bits(got[0]), bits(ev)), (name, seed)
        assert np.array_equal(bits(got[1]), bits(fl)), (name, seed)
        assert np.array_equal(got[2], mk.astype(np.float32)), (name, seed)
        n += 1
    assert n == len(golden["cases"]) >= 60


def test_torch_transforms_equal_the_reference(golden):
    """Calling the transforms on (events, flow, mask) does what the reference does - same draws from the same generators, the drop's
    rand_like included, same values, the mask bool exactly where the reference's is; and with the recorded field as `drop_u`."""
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    for name, seed, inputs, _, q, u, (ev, fl, mk, mk_is_bool) in cases(golden):
        for drop_u in ((None,) if u is None else (None, torch.from_numpy(u))):
            x = tuple(torch.from_numpy(a.copy()) for a in inputs)
            seeded(seed)
            e, f, m = A.build_chain(D, name)(x) if drop_u is None else A.build_chain(D, name)(x, drop_u)
            assert np.array_equal(bits(e.numpy()), bits(ev)) and np.array_equal(bits(f.numpy()), bits(fl)), (name, seed)
            assert (m.dtype == torch.bool) == mk_is_bool and np.array_equal(m.numpy().astype(np.uint8), mk), (name, seed)
            assert all(torch.equal(a, torch.from_numpy(b)) for a, b in zip(x, inputs))                   # the inputs are left as they were


def test_preserve_mosaicing_pattern_and_center_origin():
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    for seed in range(40):
        seeded(seed)
        i, j = D.RandomCrop((8, 10), preserve_mosaicing_pattern=True).origin(20, 30)
        random.seed(seed)
        a, b = random.randint(0, 12), random.randint(0, 20)
        assert (i, j) == (a + a % 2, b + b % 2) and i % 2 == 0 and j % 2 == 0
    assert D.CenterCrop((8, 10)).origin(11, 13) == (2, 2)                       # round(1.5): half to even
    assert D.CenterCrop((8, 10)).origin(10, 16) == (1, 3) and D.CenterCrop((8, 10), True).origin(10, 16) == (2, 4)
    assert D.CenterCrop(8).size == (8, 8) and D.RandomCrop((8, 10)).origin(8, 10) == (0, 0)


def test_refused_chains():
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    H, V, crop, drop = D.Random_horizontal_flip(), D.Random_vertical_flip(), D.RandomCrop((8, 10)), D.Random_event_drop()
    for chain in ([H, crop], [drop, H], [crop, drop, V], [H, H], [crop, crop, H], [drop, drop], [H, V, crop], [crop, H, object()]):
        with pytest.raises(ValueError, match="accepted chain is .*Crop.*flip.*drop"):
            D.Compose(chain).sample(A.SHAPE)
    for chain in ([], [crop], [H], [V, H], [crop, V, H, drop], [D.CenterCrop((8, 10)), drop]):
        D.Compose(chain).sample(A.SHAPE)
    with pytest.raises(NotImplementedError):
        D.RandomRotationFlip((0, 0), 0.5, 0.5)


def test_philox_restatement_equals_known_answers(golden):
    """Philox4x32-10 blocks against answers from an independent implementation.  No file of the published known-answer vectors was found
    in the build environment (numpy ships Philox4x64's only), so the fixture holds the output of ATen's at::philox_engine
    (torch/include/ATen/core/PhiloxRNGEngine.h) compiled on the host by tests/golden/make_golden_augment.py - for the all-zero and all-one
    counter and key, the pi-digit counter and key, and three more.  The engine's counter is (offset, subsequence), its key the seed."""
    kin, kout = golden["philox_kat_in"], golden["philox_kat_out"]
    assert len(kin) == 6 and kout.shape == (6, 4) and not kin[0].any() and (kin[1] == 2 ** 64 - 1).all()
    for (seed, sub, off), want in zip(kin.tolist(), kout.tolist()):
        got = A.philox4x32_10((off & 0xFFFFFFFF, off >> 32, sub & 0xFFFFFFFF, sub >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(w) for w in got] == want, (seed, sub, off)
    # the kernel's field: cell i takes word i & 3 of block i >> 2 at (seed, offset) - here seed 1234, offset 5: block 0 is row 3 above
    # with subsequence = the kernel's offset and engine offset = the block number
    seed, sub, off = kin[3].tolist()
    assert off == 5 and sub == 0
    blocks = [A.philox4x32_10((blk, 0, 5, 0), (1234, 0)) for blk in range(3)]
    u = A.philox_uniform(12, 1234, 5)
    assert u.dtype == np.float32
    assert [float(v) for v in u] == [float(np.float32(int(blocks[i >> 2][i & 3]) >> 8) * np.float32(2.0 ** -24)) for i in range(12)]
    assert A.philox_uniform(4, 5, 0).tolist() != u[:4].tolist()


@pytest.mark.parametrize("q", [0.1, 0.5])
def test_philox_uniform_distribution(q):
    """The share of u > q over 2^16 cells lies inside the 5-sigma binomial interval around 1 - q (u sits on a 2^-24 grid: the grid's
    effect on the probability, below 2^-24, is far inside the interval)."""
    n = 1 << 16
    u = A.philox_uniform(n, seed=20240517, offset=3)
    assert u.min() >= 0.0 and u.max() < 1.0
    kept = int((u > np.float32(q)).sum())
    sigma = math.sqrt(n * q * (1 - q))
    print(f"q {q}: kept {kept} of {n}, expected {n * (1 - q):.0f} +- {5 * sigma:.0f}")
    assert abs(kept - n * (1 - q)) <= 5 * sigma


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_and_bound():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    assert "typedef struct SdfAugmentChunkDesc" in hdr and "Added to SDF_VERSION 107 (no existing entry changed)" in hdr
    assert hip.SIGNATURES["sdf_augment_chunk_workspace_bytes"] == (C.c_int64, (C.c_int,))
    assert hip.SIGNATURES["sdf_augment_chunk_fwd"] == (C.c_int, (C.POINTER(hip.AugmentChunkDesc), C.c_void_p))
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107         # (additive exports: the version stays)
    assert int(re.search(r"#define\s+SDF_AUGMENT_MAX_B\s+(\d+)", hdr).group(1)) == hip.AUGMENT_MAX_B == 64
    names = list(hip.SIGNATURES)
    assert names.index("sdf_augment_chunk_fwd") == names.index("sdf_prepare_chunk_workspace_bytes") - 1          # beside prepare_chunk


def test_argument_errors_of_the_new_entry_points():
    """Dummy pointers: every refusal comes before any launch, so this needs no GPU."""
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.lib()
    p = 0x10000
    assert lib.sdf_augment_chunk_workspace_bytes(1) == 8 and lib.sdf_augment_chunk_workspace_bytes(64) == 512
    assert lib.sdf_augment_chunk_workspace_bytes(0) == 0 and lib.sdf_augment_chunk_workspace_bytes(65) == 0
    assert lib.sdf_augment_chunk_fwd(None, None) == hip.E_NULL
    B, Hs, Ws, h, w = 3, 11, 13, 8, 10

    def ac(origin=None, flag=None, **kw):
        d = hip.AugmentChunkDesc()
        d.voxel = d.label = d.valid = d.out = d.label_out = d.mask_out = d.workspace = p
        d.workspace_bytes, d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.norm = 256, B, 2, Hs, Ws, h, w, 1
        for b in range(64):                                       # (entries beyond B are not looked at)
            d.oy[b], d.ox[b], d.flags[b], d.drop_q[b] = (1, 2, b & 3, -1.0) if b < B else (-5, 1 << 20, 255, 0.5)
        for k, v in kw.items():
            setattr(d, k, v)
        if origin is not None:
            b, oy, ox = origin
            d.oy[b], d.ox[b] = oy, ox
        if flag is not None:
            d.flags[flag[0]] = flag[1]
        return lib.sdf_augment_chunk_fwd(C.byref(d), None)
    # a NULL required pointer; an input without its output and the reverse
    assert ac(voxel=None) == hip.E_NULL and ac(out=None) == hip.E_NULL and ac(workspace=None) == hip.E_NULL
    assert ac(label_out=None) == hip.E_NULL and ac(label=None) == hip.E_NULL                 # label without label_out, and the reverse
    assert ac(mask_out=None) == hip.E_NULL and ac(valid=None) == hip.E_NULL
    assert ac(valid=None, mask_out=None, mask_events=1) == hip.E_NULL                        # nothing to multiply
    # the batch
    assert ac(B=0) == hip.E_SHAPE and ac(B=65) == hip.E_SHAPE and ac(B=-1) == hip.E_SHAPE
    assert ac(bins=0) == hip.E_SHAPE and ac(Hs=0) == hip.E_SHAPE
    # origins: the last valid one passes the geometry check (refused later, for the pointer), one past it does not - any sample
    assert ac(origin=(B - 1, Hs - h, Ws - w), out=p + 2) == hip.E_ALIGN and ac(origin=(0, 0, 0), out=p + 2) == hip.E_ALIGN
    for b in range(B):
        assert ac(origin=(b, Hs - h + 1, 0)) == hip.E_SHAPE and ac(origin=(b, 0, Ws - w + 1)) == hip.E_SHAPE
        assert ac(origin=(b, -1, 0)) == hip.E_SHAPE and ac(origin=(b, 0, -1)) == hip.E_SHAPE
        assert ac(origin=(b, 2 ** 31 - 1, 0)) == hip.E_SHAPE and ac(origin=(b, 0, -2 ** 31)) == hip.E_SHAPE
    assert ac(crop_h=0) == hip.E_SHAPE and ac(crop_h=Hs + 1) == hip.E_SHAPE                  # half a crop; a crop larger than the volume
    assert ac(crop_h=0, crop_w=0) == hip.E_SHAPE                                             # the whole volume: origins are 0
    # selectors
    assert ac(norm=2) == hip.E_DTYPE and ac(norm=-1) == hip.E_DTYPE                          # "std" is the torch function's
    assert ac(flag=(1, 4)) == hip.E_DTYPE
    # alignment, workspace
    assert ac(voxel=p + 2) == hip.E_ALIGN and ac(label=p + 1) == hip.E_ALIGN and ac(valid=p + 2) == hip.E_ALIGN
    assert ac(drop_u=p + 2) == hip.E_ALIGN
    assert ac(label_out=p + 2) == hip.E_ALIGN and ac(mask_out=p + 2) == hip.E_ALIGN and ac(event_mask=p + 2) == hip.E_ALIGN
    assert ac(workspace=p + 4) == hip.E_ALIGN
    assert ac(workspace_bytes=8 * B - 1) == hip.E_SHAPE


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    from sdformerflow_amd import hip, train
    v = torch.zeros(2, 3, 11, 13)
    with pytest.raises(hip.SdfError):
        hip.augment_chunk(v, None, None, (8, 10), (0, 0), 0)
    cfg = {"model": {"norm_input": "minmax", "encoding": "voxel"}, "loader": {"polarity": True, "crop": [8, 10]}, "data": {"spike_th": None}}
    with pytest.raises(hip.SdfError):
        train.prepare_train_item(v, torch.zeros(2, 2, 11, 13), torch.ones(2, 11, 13), cfg, None)


def test_torch_fallback_of_prepare_train_item():
    """`norm_input: std` is served by the torch sequence - on the CPU here: CenterCrop(loader.crop) for `transform` None, the split,
    mean / std, and mask * event_mask."""
    from sdformerflow_amd import harness, train
    from sdformerflow_amd.DSEC_dataloader import data_augmentation as D
    g = torch.Generator().manual_seed(5)
    v = torch.randn((2, 3, 11, 13), generator=g) * (torch.rand((2, 3, 11, 13), generator=g) < 0.3)
    label, mask = torch.randn((2, 2, 11, 13), generator=g), (torch.rand((2, 11, 13), generator=g) < 0.7)
    cfg = {"model": {"norm_input": "std", "encoding": "voxel"}, "loader": {"polarity": True, "crop": [8, 10]}, "data": {"spike_th": None},
           "metrics": {"mask_events": True}}
    x, lab, m = train.prepare_train_item(v, label, mask, cfg, None)
    want = harness.prepare_chunk(v[..., 2:10, 2:12], "std", None, True)
    assert torch.equal(x, want) and torch.equal(lab, label[..., 2:10, 2:12])
    assert m.dtype == torch.float32 and torch.equal(m, mask[:, None, 2:10, 2:12].float() * want.sum(1).sum(1, keepdim=True).bool())
    t = train.train_transform({"loader": {"augment_prob": [0.5, 0.25, 0.0], "crop": [8, 10]}})
    assert [type(a) for a in t.transforms] == [D.RandomCrop, D.Random_horizontal_flip, D.Random_vertical_flip]
    assert t.transforms[0].size == (8, 10) and (t.transforms[1].p, t.transforms[2].p) == (0.5, 0.25)
    assert [type(a) for a in train.train_transform({"loader": {"augment_prob": [1, 1], "crop": [8, 10]}}, finetune=True).transforms][0] is D.Random_horizontal_flip
