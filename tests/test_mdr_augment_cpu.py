"""The MDR training front end without a GPU: `DenseSparseAugmentor` of sdformerflow_amd.MDR_dataloader.loader_utils - its draws, its
`__call__` and the valid rule - against the reference's own outputs (tests/golden/mdr_augment.npz, made by
tests/golden/make_golden_mdr_augment.py from the reference's class; the interpolated values in it are `resize_linear`'s, cv2 being
absent where it was made); `resize_linear` against a float64 evaluation of its taps and against torch's bilinear interpolation; the
torch sequence of train.prepare_mdr_item_torch against the numpy restatement; and the new entry points in the header, in the binding's
signature table, and their argument checks (refused before any launch)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mdr_augment_cases as M  # noqa: E402

from sdformerflow_amd.MDR_dataloader import loader_utils as L  # noqa: E402

NEW = ("sdf_augment_resize_workspace_bytes", "sdf_augment_resize_fwd")
U = 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "mdr_augment.npz"))
    assert tuple(z["frame"]) == M.FRAME and tuple(z["crop"]) == M.CROP and tuple(z["scales"]) == (M.MIN_SCALE, M.MAX_SCALE)
    for k in (0, 1):                                               # the inputs are the seeded ones
        vols, flow = M.fixture_inputs(k)
        assert np.array_equal(z[f"in{k}_vols"], np.stack(vols)) and z[f"in{k}_flow"].tobytes() == flow.tobytes()
    return z


def augmentor():
    return L.DenseSparseAugmentor(list(M.CROP), min_scale=M.MIN_SCALE, max_scale=M.MAX_SCALE, do_flip=True)


def test_constructor_and_attributes():
    a = L.DenseSparseAugmentor([256, 256])
    assert (a.crop_size, a.min_scale, a.max_scale, a.do_flip) == ([256, 256], -0.2, 0.5, False)
    assert (a.spatial_aug_prob, a.stretch_prob, a.max_stretch, a.h_flip_prob, a.v_flip_prob) == (0.8, 0.8, 0.2, 0.5, 0.1)
    src = open(L.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(cv2|torchvision|pandas)", src, flags=re.M)


def test_fixture_shows_every_outcome(golden):
    rec = [M.params_of(r, L.ResizeParams) for r in golden["records"]]
    floor = max((M.CROP[0] + 8) / M.FRAME[0], (M.CROP[1] + 8) / M.FRAME[1])
    assert {p.resized for p in rec} == {p.hflip for p in rec} == {p.vflip for p in rec} == {False, True}
    assert any(p.scale_x != p.scale_y for p in rec) and any(p.scale_x == p.scale_y for p in rec)          # stretched and not
    assert any(floor in (p.scale_x, p.scale_y) for p in rec)                                              # clipped from below
    assert any(p.resized and min(p.scale_x, p.scale_y) < 1 for p in rec) and any(p.resized and max(p.scale_x, p.scale_y) > 1 for p in rec)
    assert {0, 1} <= {p.y0 / (p.size[0] - M.CROP[0] - 1) for p in rec} and {0, 1} <= {p.x0 / (p.size[1] - M.CROP[1] - 1) for p in rec}
    assert bool(golden["cv2_is_restated"])


def test_sample_reproduces_the_reference_draws(golden):
    """`sample` under the fixture's seeds gives every record - the scales bit-equal as float64 - and leaves numpy's generator where the
    reference's call left it; `sample_batch` is the same draws item after item."""
    aug = augmentor()
    for (seed, _), row in zip(golden["seeds"].tolist(), golden["records"]):
        np.random.seed(seed)
        p = aug.sample(M.FRAME)
        assert isinstance(p.scale_x, float) and M.record_of(p).tobytes() == row.tobytes(), (seed, p)
        assert p.size == (L.resize_size(M.FRAME, p.scale_x, p.scale_y) if p.resized else M.FRAME)
        assert np.random.rand() == float(golden[f"s{seed}_after"]), seed
    np.random.seed(3)
    batch = aug.sample_batch(3, M.FRAME)
    np.random.seed(3)
    assert batch == [aug.sample(M.FRAME) for _ in range(3)] and len({(p.y0, p.x0, p.scale_x) for p in batch}) == 3


def test_call_reproduces_the_reference_outputs(golden):
    aug = augmentor()
    for seed, k in golden["seeds"].tolist():
        vols, flow = M.fixture_inputs(k)
        np.random.seed(seed)
        got = aug(*[v.copy() for v in vols], flow.copy())
        assert np.random.rand() == float(golden[f"s{seed}_after"])
        for name, a in zip(("img1", "img2", "dimg1", "dimg2", "flow"), got):
            want = golden[f"s{seed}_{name}"]
            assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), (seed, name)
            assert a.flags["C_CONTIGUOUS"]
        untouched = not (golden[f"s{seed}_flow"].dtype == np.float64)
        p = M.params_of(golden["records"][[s for s, _ in golden["seeds"].tolist()].index(seed)], L.ResizeParams)
        assert untouched == (not p.resized and not p.hflip and not p.vflip)
        # the item: one rounding of the flow, and the valid rule in the flow's own precision
        with np.errstate(invalid="ignore"):
            assert torch.from_numpy(got[4]).float().numpy().tobytes() == golden[f"s{seed}_item_flow"].transpose(1, 2, 0).tobytes()
            assert np.array_equal(L.flow_valid(got[4]).astype(np.float32), golden[f"s{seed}_valid"])
        for v, w in zip(vols, M.fixture_inputs(k)[0]):
            assert np.array_equal(v, w)                            # the inputs are left as they were


def test_restatement_of_the_kernel_equals_the_reference_item(golden):
    """tests/mdr_augment_cases.py gather - what the GPU tests hold the kernel to - under the recorded parameters gives the item's
    dense volumes, flow and valid (NaN-aware on the flow)."""
    aug = augmentor()
    invalid = 0
    for (seed, k), row in zip(golden["seeds"].tolist(), golden["records"]):
        vols, flow = M.fixture_inputs(k)
        p = M.params_of(row, L.ResizeParams)
        old, new, fl = (np.ascontiguousarray(a.transpose(2, 0, 1))[None] for a in (vols[2], vols[3], flow))
        ev, f, mk = M.gather(aug, old, new, fl, [p])
        want = np.concatenate((golden[f"s{seed}_dimg1"], golden[f"s{seed}_dimg2"]), axis=2).transpose(2, 0, 1)
        assert ev.dtype == np.float32 and ev[0].tobytes() == np.ascontiguousarray(want).tobytes(), seed
        assert M.same_bits_or_nan(f[0], golden[f"s{seed}_item_flow"]), seed
        # (the reference's norm is fp32 for an item nothing touched - the documented divergence, which these magnitudes do not reach)
        assert np.array_equal(mk[0, 0], golden[f"s{seed}_valid"]), seed
        invalid += int((mk == 0).sum())
    assert 0 < invalid < 80 * len(golden["records"])               # some pixels of the crops are invalid, not all


def test_valid_rule():
    f = np.zeros((2, 4, 2), np.float64)
    f[0, 0] = (1.0, 0.0)
    f[0, 1] = (0.0, 0.0)
    f[0, 2] = (np.inf, 1.0)
    f[0, 3] = (1.0, -np.inf)
    f[1, 0] = (np.nan, 1.0)
    f[1, 1] = (0.0, -2.0)
    f[1, 2] = (-0.0, 0.0)
    f[1, 3] = (1e-30, 0.0)
    with np.errstate(invalid="ignore"):
        assert L.flow_valid(f).tolist() == [[True, False, False, False], [False, True, False, True]]
        assert L.flow_valid(f.astype(np.float32)).tolist()[1][3] is False      # fp32 norm: 1e-60 underflows (the reference's untouched item)


def resize64(img, fx, fy):
    """The same taps and weights evaluated in float64."""
    H, W = img.shape[:2]
    h, w = L.resize_size((H, W), fx, fy)
    x0, x1, ax = L._linear_axis(W, w, fx)
    y0, y1, ay = L._linear_axis(H, h, fy)
    i, ax, ay = img.astype(np.float64), ax.astype(np.float64)[None, :, None], ay.astype(np.float64)[:, None, None]
    rows = i[:, x0] * (1 - ax) + i[:, x1] * ax
    return rows[y0] * (1 - ay) + rows[y1] * ay


def image(H, W, C, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((H, W, C)) * (g.random((H, W, C)) < 0.6)).astype(np.float32)


def test_resize_linear_identity_size_and_axis_rule():
    img = image(11, 13, 4, 0) + np.float32(0)                                         # (no negative zero)
    img[5, 5, 1] = np.float32(1e-40)
    assert L.resize_linear(img, 1.0, 1.0).tobytes() == img.tobytes()                 # bit for bit, a denormal included
    img[3, 4, 0] = -0.0                                                              # S (1 - 0) + S' 0 = -0 + 0: the rule's own +0
    assert L.resize_linear(img, 1.0, 1.0)[3, 4, 0].tobytes() == np.float32(0).tobytes()
    assert L.resize_linear(img[:, :, 1], 1.0, 1.0).tobytes() == np.ascontiguousarray(img[:, :, 1]).tobytes()        # a plain (H, W) image
    assert L.resize_size((10, 10), 1.25, 1.05) == (10, 12) and L.resize_size((10, 2), 1.25, 1.15) == (12, 2)      # 12.5 -> 12, 10.5 -> 10; 2.5 -> 2
    assert L.resize_linear(img, 1.3, 0.7).shape == (8, 17, 4) and L.resize_linear(img, 1.3, 0.7).dtype == np.float32
    # upscaling by 2: c = d / 2 - 0.25 -> taps (0, 0), (0, 1), (0, 1), (1, 2) ... with weights 0 (clamped), .25, .75, .25, and the last
    # destination clamps to the last source element at weight 0
    i0, i1, a = L._linear_axis(4, 8, 2.0)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert a.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.0] and a.dtype == np.float32
    i0, i1, a = L._linear_axis(8, 4, 0.5)                                              # downscaling by 2: c = 2 d + 0.5
    assert i0.tolist() == [0, 2, 4, 6] and i1.tolist() == [1, 3, 5, 7] and a.tolist() == [0.5] * 4
    with pytest.raises(ValueError):
        L.resize_linear(img.astype(np.float64), 1.0, 1.0)


@pytest.mark.parametrize("H,W,fx,fy", [(13, 17, 1.37, 1.21), (13, 17, 0.93, 0.95), (26, 35, 2.0, 1.0), (260, 346, 1.2311, 1.0802),
                                       (260, 346, 1.02, 0.99)])
def test_resize_linear_against_float64(H, W, fx, fy):
    """Two passes of two products and a sum, each rounded once: within 4 units of 2^-23 max|src| of the float64 evaluation."""
    img = image(H, W, 4, 1)
    err = np.abs(L.resize_linear(img, fx, fy) - resize64(img, fx, fy)).max() / (U * np.abs(img).max())
    print(f"{H} x {W} at ({fx}, {fy}): {err:.3f} of the 4 units allowed")
    assert err <= 4.0


@pytest.mark.parametrize("H,W,fx,fy", [(13, 17, 1.30, 1.25), (13, 17, 0.95, 0.93), (260, 346, 1.2168, 1.081)])
def test_resize_linear_against_torch_bilinear(H, W, fx, fy):
    """An independent implementation: torch's bilinear interpolation (align_corners False, the scale factors used as given) at
    scales where floor(n f) == rint(n f) on both axes, so the sizes agree.  torch forms the coordinate in float32: its error, at most
    about (Hs + Ws) 2^-23 per axis pair, times the largest neighbour difference (<= 2 max|src|) bounds the deviation."""
    assert np.floor(H * fy) == np.rint(H * fy) and np.floor(W * fx) == np.rint(W * fx)
    img = image(H, W, 4, 2)
    got = L.resize_linear(img, fx, fy)
    ref = torch.nn.functional.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], scale_factor=(fy, fx), mode="bilinear",
                                          align_corners=False, recompute_scale_factor=False)[0].permute(1, 2, 0).numpy()
    assert ref.shape == got.shape
    bound = 2 * (H + W)
    err = np.abs(got - ref).max() / (U * np.abs(img).max())
    print(f"{H} x {W} at (fx {fx}, fy {fy}): {err:.1f} of the {bound} units allowed, bit-equal share {(got == ref).mean():.3f}")
    assert err <= bound


def test_torch_sequence_equals_the_restatement():
    """train.prepare_mdr_item_torch on CPU tensors against the numpy restatement, bit for bit (NaN-aware on the flow): both chunk
    counts, every record of the fixture plus a flip without a resize, min-max and mask_events."""
    from sdformerflow_amd import train
    z = np.load(os.path.join(ROOT, "tests", "golden", "mdr_augment.npz"))
    aug = augmentor()
    rec = [M.params_of(r, L.ResizeParams) for r in z["records"]] + [L.ResizeParams(False, 1.2, 0.9, M.FRAME, True, True, 13, 0)]
    vols, flow = M.fixture_inputs(0)
    B = len(rec)
    g = np.random.default_rng(5)
    old, new = (np.stack([np.roll(vols[i], b, axis=0) for b in range(B)]).transpose(0, 3, 1, 2).copy() for i in (2, 3))
    fl = np.stack([np.roll(flow, b, axis=1) for b in range(B)]).transpose(0, 3, 1, 2).copy()
    new *= g.uniform(0.5, 2.0, (B, 1, 1, 1)).astype(np.float32)
    for chunks, norm, th, me in ((2, "minmax", None, True), (1, None, 0.5, False), (2, "minmax", 0.5, True)):
        cfg = {"model": {"norm_input": norm, "encoding": "voxel"}, "loader": {"polarity": True, "crop": list(M.CROP)},
               "data": {"spike_th": th, "num_chunks": chunks}, "metrics": {"mask_events": me}}
        sample = {"d_event_volume_old": torch.from_numpy(old), "d_event_volume_new": torch.from_numpy(new), "flow": torch.from_numpy(fl)}
        x, lab, m = train.prepare_mdr_item_torch(sample, cfg, aug, rec)
        want = M.augment_resize(aug, old if chunks == 2 else None, new, fl, rec, norm=norm, spike_th=th, mask_events=me)
        assert x.shape == (B, 3 * chunks, 2, *M.CROP) and x.dtype == lab.dtype == m.dtype == torch.float32
        # (torch's relu keeps a -0 on the CPU and makes it +0 on the GPU, as the restatement does: values here, bits in the GPU tests)
        assert np.array_equal(x.numpy(), want["out"]) and M.same_bits_or_nan(lab.numpy(), want["label"])
        assert np.array_equal(m.numpy(), want["mask"]) and 0 < m.sum() < m.numel()
    # drawn inside: the generator ends where B calls of the augmentor leave it; std is served
    cfg["model"]["norm_input"] = "std"
    np.random.seed(11)
    a = train.prepare_mdr_item(sample, cfg, aug)
    after = np.random.rand()
    np.random.seed(11)
    b = train.prepare_mdr_item_torch(sample, cfg, aug, aug.sample_batch(B, M.FRAME))
    assert after == np.random.rand() and all(M.same_bits_or_nan(p.numpy(), q.numpy()) for p, q in zip(a, b))
    t = train.mdr_train_augmentor({"loader": {"crop": [256, 256], "min_scale": -0.1, "max_scale": 0.4}})
    assert isinstance(t, L.DenseSparseAugmentor) and (t.crop_size, t.min_scale, t.max_scale, t.do_flip) == ([256, 256], -0.1, 0.4, True)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_and_bound():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    assert "typedef struct SdfAugmentResizeDesc" in hdr
    section = hdr[hdr.index("An MDR loader item"):hdr.index("typedef struct SdfAugmentResizeDesc")]
    assert "Added to SDF_VERSION 107 (no existing entry changed)" in section
    assert hip.SIGNATURES["sdf_augment_resize_workspace_bytes"] == (C.c_int64, (C.c_int,))
    assert hip.SIGNATURES["sdf_augment_resize_fwd"] == (C.c_int, (C.POINTER(hip.AugmentResizeDesc), C.c_void_p))
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107         # (additive exports: the version stays)
    assert int(re.search(r"#define\s+SDF_AUGMENT_MAX_B\s+(\d+)", hdr).group(1)) == hip.AUGMENT_MAX_B == 64
    body = re.search(r"typedef struct SdfAugmentResizeDesc \{(.*?)\} SdfAugmentResizeDesc;", hdr, flags=re.S).group(1)
    members = re.findall(r"(\w+)(?:\[64\])?\s*[,;]", body)
    assert members == [f for f, _ in hip.AugmentResizeDesc._fields_]
    assert "const double* scale_x;" in body and "const double* scale_y;" in body
    names = list(hip.SIGNATURES)
    assert names.index("sdf_augment_resize_fwd") == names.index("sdf_augment_chunk_workspace_bytes") - 1           # beside its sibling


def test_argument_errors_of_the_new_entry_points():
    """Dummy device pointers: every refusal comes before any launch, so this needs no GPU.  The order of sdf_augment_chunk_fwd's
    family: NULL descriptor (and the host arrays the geometry check reads), geometry of every sample, selectors, NULL pointers,
    workspace size, alignment."""
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.lib()
    p = 0x10000
    assert lib.sdf_augment_resize_workspace_bytes(1) == 8 and lib.sdf_augment_resize_workspace_bytes(64) == 512
    assert lib.sdf_augment_resize_workspace_bytes(0) == 0 and lib.sdf_augment_resize_workspace_bytes(65) == 0
    assert lib.sdf_augment_resize_fwd(None, None) == hip.E_NULL
    B, Hs, Ws, h, w = 3, 21, 25, 8, 10
    sx, sy = 1.1330065123464295, 0.9186546633217058
    rh, rw = int(np.rint(Hs * sy)), int(np.rint(Ws * sx))
    assert (rh, rw) == (19, 28)

    def rz(sample=None, scales=None, **kw):
        d = hip.AugmentResizeDesc()
        d.vox_old = d.vox_new = d.flow = d.out = d.label_out = d.mask_out = d.workspace = p
        d.workspace_bytes, d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.norm, d.num_chunks = 256, B, 2, Hs, Ws, h, w, 1, 2
        xs, ys = (C.c_double * 64)(*([sx] * 64)), (C.c_double * 64)(*([sy] * 64))
        for b in range(64):                                       # (entries beyond B are not looked at)
            row = (1, rh, rw, 2, 3, b & 3) if b < B - 1 else (0, Hs, Ws, 2, 3, 1) if b == B - 1 else (1, -7, 1 << 30, -5, 1 << 20, 255)
            d.resized[b], d.rh[b], d.rw[b], d.oy[b], d.ox[b], d.flags[b] = row
            if b >= B:
                xs[b] = ys[b] = float("nan")
        if scales is not None:
            b, x, y = scales
            xs[b], ys[b] = x, y
        d.scale_x, d.scale_y = C.addressof(xs), C.addressof(ys)
        for k, v in kw.items():
            setattr(d, k, v)
        if sample is not None:
            b, fields = sample
            for k, v in fields.items():
                getattr(d, k)[b] = v
        return lib.sdf_augment_resize_fwd(C.byref(d), None)
    ok = hip.E_ALIGN                                               # a call that passes every check but the last: out misaligned
    assert rz(out=p + 2) == ok
    # NULL: the host arrays first, then the required pointers; the old volume only with two chunks
    assert rz(scale_x=None) == hip.E_NULL and rz(scale_y=None, B=0) == hip.E_NULL
    for name in ("vox_new", "flow", "out", "label_out", "mask_out", "workspace"):
        assert rz(**{name: None}) == hip.E_NULL, name
    assert rz(vox_old=None) == hip.E_NULL and rz(vox_old=None, num_chunks=1, out=p + 2) == ok
    # the batch and the dimensions
    assert rz(B=0) == hip.E_SHAPE and rz(B=65) == hip.E_SHAPE and rz(B=-1) == hip.E_SHAPE
    assert rz(bins=0) == hip.E_SHAPE and rz(Hs=0) == hip.E_SHAPE and rz(Ws=0) == hip.E_SHAPE
    assert rz(crop_h=0) == hip.E_SHAPE and rz(crop_w=0) == hip.E_SHAPE and rz(crop_h=0, crop_w=0) == hip.E_SHAPE
    # per sample, every sample: origins - the last valid one passes, one past it does not
    assert rz(sample=(0, dict(oy=rh - h, ox=rw - w)), out=p + 2) == ok and rz(sample=(B - 1, dict(oy=Hs - h, ox=Ws - w)), out=p + 2) == ok
    assert rz(sample=(1, dict(oy=0, ox=0)), out=p + 2) == ok
    for b in range(B):
        top = (rh - h, rw - w) if b < B - 1 else (Hs - h, Ws - w)
        assert rz(sample=(b, dict(oy=top[0] + 1))) == hip.E_SHAPE and rz(sample=(b, dict(ox=top[1] + 1))) == hip.E_SHAPE
        assert rz(sample=(b, dict(oy=-1))) == hip.E_SHAPE and rz(sample=(b, dict(ox=-1))) == hip.E_SHAPE
        assert rz(sample=(b, dict(oy=2 ** 31 - 1))) == hip.E_SHAPE and rz(sample=(b, dict(ox=-2 ** 31))) == hip.E_SHAPE
    # ... a resized size that is not rint(Hs scale_y) x rint(Ws scale_x); a sample that is not resized at another size
    for b in range(B - 1):
        assert rz(sample=(b, dict(rh=rh + 1))) == hip.E_SHAPE and rz(sample=(b, dict(rw=rw - 1))) == hip.E_SHAPE
        assert rz(sample=(b, dict(rh=Hs, rw=Ws))) == hip.E_SHAPE
    assert rz(sample=(B - 1, dict(rh=rh, rw=rw))) == hip.E_SHAPE and rz(sample=(B - 1, dict(resized=1))) == hip.E_SHAPE
    assert rz(scales=(B - 1, float("nan"), -1.0), out=p + 2) == ok               # (its scales are not looked at)
    # ... half to even: 10 x 1.25 = 12.5 -> 12, 10 x 1.05 = 10.5 -> 10
    even = dict(Hs=10, Ws=10, crop_h=4, crop_w=4, B=1)
    assert rz(scales=(0, 1.25, 1.05), sample=(0, dict(rh=10, rw=12)), out=p + 2, **even) == ok
    assert rz(scales=(0, 1.25, 1.05), sample=(0, dict(rh=11, rw=13)), **even) == hip.E_SHAPE
    # ... a resized size smaller than the crop
    small = dict(sample=(0, dict(rh=int(np.rint(Hs * 0.3)), rw=rw, oy=0)), scales=(0, sx, 0.3))
    assert int(np.rint(Hs * 0.3)) < h and rz(**small) == hip.E_SHAPE
    # ... a scale that is not finite and positive
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert rz(scales=(0, bad, sy)) == hip.E_SHAPE and rz(scales=(1, sx, bad)) == hip.E_SHAPE, bad
    # selectors come behind the geometry and before the pointers
    assert rz(norm=2) == hip.E_DTYPE and rz(norm=-1) == hip.E_DTYPE and rz(norm=2, out=None) == hip.E_DTYPE
    assert rz(num_chunks=0) == hip.E_DTYPE and rz(num_chunks=3) == hip.E_DTYPE
    assert rz(sample=(1, dict(flags=4))) == hip.E_DTYPE and rz(sample=(1, dict(flags=4)), B=0) == hip.E_SHAPE
    # workspace, alignment
    assert rz(workspace_bytes=8 * B - 1) == hip.E_SHAPE and rz(workspace_bytes=8 * B - 1, out=p + 2) == hip.E_SHAPE
    for name in ("vox_old", "vox_new", "flow", "label_out", "mask_out", "event_mask"):
        assert rz(**{name: p + 2}) == hip.E_ALIGN, name
    assert rz(workspace=p + 4) == hip.E_ALIGN


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    from sdformerflow_amd import hip, train
    v, f = torch.zeros(2, 3, 21, 25), torch.zeros(2, 2, 21, 25)
    p = L.ResizeParams(False, 1.0, 1.0, (21, 25), False, False, 0, 0)
    with pytest.raises(hip.SdfError):
        hip.augment_resize_chunk(v, v, f, (8, 10), p)
    cfg = {"model": {"norm_input": "minmax", "encoding": "voxel"}, "loader": {"polarity": True}, "data": {"spike_th": None, "num_chunks": 2}}
    with pytest.raises(hip.SdfError):
        train.prepare_mdr_item({"d_event_volume_old": v, "d_event_volume_new": v, "flow": f}, cfg, augmentor(), [p, p])
    with pytest.raises(ValueError):
        train.prepare_mdr_item({"d_event_volume_old": v, "d_event_volume_new": v, "flow": f}, {**cfg, "data": {"num_chunks": 3}}, augmentor())
