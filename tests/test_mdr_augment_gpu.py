"""hip.augment_resize_chunk (csrc/prepare_chunk.hip, sdf_augment_resize_fwd) on the GPU: bit for bit against its numpy restatement
(tests/mdr_augment_cases.py: the package's DenseSparseAugmentor.apply per sample, then the preparation of tests/augment_cases.py) and
against the torch composition (train.prepare_mdr_item_torch); and train.train_step_from_mdr_item beside train.train_step.

Every buffer a call touches is a window between guard bytes, checked after the call.  The flow is compared bit for bit where it is a
number and as "NaN where the reference has NaN" elsewhere: the sign and payload of a NaN that inf * 0 generates are the
implementation's (IEEE 754 6.2), and the host's differ from the GPU's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import hip, train
from sdformerflow_amd.MDR_dataloader import loader_utils as L

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mdr_augment_cases as M  # noqa: E402
from routes_common import short  # noqa: E402
from test_augment_gpu import AtenOps, Guarded, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, F, Hs, Ws), crop: less than one workgroup per sample | several | 64 workgroups per sample
SHAPES = (((2, 3, 21, 25), (8, 10)), ((3, 5, 37, 41), (24, 28)), ((2, 5, 140, 150), (128, 128)))
GOLDEN = np.load(os.path.join(HERE, "golden", "mdr_augment.npz"))


def run_kernel(vox_old, vox_new, flow, crop, params, norm=None, per_sample=False, spike_th=None, mask_events=False, want_event_mask=True):
    """sdf_augment_resize_fwd called directly on numpy inputs, every buffer a guarded window.  Returns the outputs as numpy arrays and
    the launch log's rows."""
    B, bins, Hs, Ws = vox_new.shape
    h, w = crop
    nF = bins * (1 + (vox_old is not None))
    lib = hip.lib()
    ws_bytes = lib.sdf_augment_resize_workspace_bytes(B)
    assert ws_bytes == 8 * B
    bufs = {"vox_new": Guarded(vox_new.nbytes, vox_new), "flow": Guarded(flow.nbytes, flow), "out": Guarded(B * nF * 2 * h * w * 4),
            "label_out": Guarded(B * 2 * h * w * 4), "mask_out": Guarded(B * h * w * 4), "workspace": Guarded(ws_bytes)}
    if vox_old is not None:
        bufs["vox_old"] = Guarded(vox_old.nbytes, vox_old)
    if want_event_mask:
        bufs["event_mask"] = Guarded(B * h * w * 4)
    d = hip.AugmentResizeDesc()
    for name, g in bufs.items():
        setattr(d, name, g.ptr())
    sx, sy = (C.c_double * 64)(*([float("nan")] * 64)), (C.c_double * 64)(*([float("nan")] * 64))
    d.scale_x, d.scale_y = C.addressof(sx), C.addressof(sy)
    d.workspace_bytes = ws_bytes
    d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.num_chunks = B, bins, Hs, Ws, h, w, 1 + (vox_old is not None)
    d.norm, d.per_sample = int(norm == "minmax"), int(per_sample)
    d.use_spike_th, d.spike_th, d.mask_events = int(spike_th is not None), float(spike_th or 0.0), int(mask_events)
    for b in range(64):                                            # (entries beyond B are not looked at)
        if b < B:
            p = params[b]
            sx[b], sy[b] = p.scale_x, p.scale_y
            d.resized[b], d.rh[b], d.rw[b], d.oy[b], d.ox[b], d.flags[b] = int(p.resized), *p.size, p.y0, p.x0, int(p.hflip) | int(p.vflip) << 1
        else:
            d.resized[b], d.rh[b], d.rw[b], d.oy[b], d.ox[b], d.flags[b] = 1, -7, 1 << 30, -9, 1 << 20, 255
    with hip.launch_log() as log:
        rc = lib.sdf_augment_resize_fwd(C.byref(d), hip._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    broken = [name for name, g in bufs.items() if not g.intact()]
    assert not broken, f"a store outside {broken}"
    got = {"out": bufs["out"].array(np.float32, (B, nF, 2, h, w)), "label": bufs["label_out"].array(np.float32, (B, 2, h, w)),
           "mask": bufs["mask_out"].array(np.float32, (B, 1, h, w)),
           "event_mask": bufs["event_mask"].array(np.float32, (B, 1, h, w)) if want_event_mask else None}
    for name, src in (("vox_old", vox_old), ("vox_new", vox_new), ("flow", flow)):                       # the inputs are left as they were
        assert src is None or np.array_equal(bufs[name].array(np.uint8, (-1,)), np.ascontiguousarray(src).view(np.uint8).reshape(-1)), name
    return got, log.rows


def make_item(shape, seed, kind="random"):
    """Two signed volumes with ~40 % zeros (negative zeros among them) and per-sample ranges, and a flow with exact zeros - single
    components and whole pixels.  `flow_cases`: an inf, a -inf and a NaN per sample as well."""
    B, F, Hs, Ws = shape
    g = np.random.Generator(np.random.PCG64(seed))

    def volume():
        v = g.uniform(-1.0, 1.0, shape) * (1.0 + g.exponential(0.5, shape))
        return np.where(g.random(shape) < 0.6, v, np.where(g.random(shape) < 0.5, 0.0, -0.0)) * (1.0 + np.arange(B)).reshape(B, 1, 1, 1)
    old, new = volume(), volume()
    if kind == "zero_sample":                                      # one sample without an event
        old[B - 1] = new[B - 1] = 0.0
    if kind == "equal":                                            # every non-zero is +-0.75: lo == hi, left unnormalised
        old, new = (np.where(v != 0.0, np.sign(v) * 0.75, 0.0) for v in (old, new))
    flow = np.where(g.random((B, 2, Hs, Ws)) < 0.9, g.normal(0.0, 5.0, (B, 2, Hs, Ws)), 0.0)
    flow = flow * (g.random((B, 1, Hs, Ws)) < 0.9)                 # pixels with both components zero
    if kind == "flow_cases":
        for b in range(B):
            for j, bad in enumerate((np.inf, -np.inf, np.nan)):
                flow[b, (b + j) % 2, g.integers(0, Hs, 6), g.integers(0, Ws, 6)] = bad
    return old.astype(np.float32), new.astype(np.float32), flow.astype(np.float32)


def make_params(idx, shape, crop, B=None):
    """The records of case `idx` over one shape.  Scales from {just large enough for the crop (below 1), 1.17, 1.3} in the four
    below / above combinations of the two axes, rotating over the samples; not resized: everybody in cases 4 and 9, every third
    sample from case 6 on; the flip word `idx` for every sample in cases 0-3, rotating afterwards; the origins (0, 0), the largest
    (which reads the clamped border taps) and an interior one, rotating."""
    _, _, Hs, Ws = shape
    h, w = crop
    low_y, low_x = (h + 2) / Hs, (w + 3) / Ws
    assert low_y < 1 and low_x < 1
    scales = [(low_x, 1.3), (1.17, low_y), (low_x, low_y), (1.3, 1.17)]
    out = []
    for b in range(shape[0] if B is None else B):
        k = b + idx
        resized = idx not in (4, 9) and not (idx >= 6 and k % 3 == 0)
        sx, sy = scales[k % 4]
        rh, rw = L.resize_size((Hs, Ws), sx, sy) if resized else (Hs, Ws)
        f = idx if idx < 4 else k % 4
        y0, x0 = [(0, 0), (rh - h, rw - w), ((rh - h) // 2, (rw - w + 1) // 2)][k % 3]
        out.append(L.ResizeParams(resized, sx, sy, (rh, rw), bool(f & 1), bool(f & 2), y0, x0))
    return out


def option_set(idx):
    """Case `idx` of 12: num_chunks 1 in cases 3, 7, 11; norm none / whole batch / per sample; spike_th none / 0.5; mask_events; the
    event mask asked for or not."""
    return dict(chunks=1 if idx % 4 == 3 else 2, norm=[None, "minmax", "minmax"][idx % 3], per_sample=idx % 3 == 2,
                spike_th=[None, 0.5][idx % 2], mask_events=bool((idx // 2) % 2), want_event_mask=idx % 4 != 1)


def check_against_restatement(item, crop, params, o):
    old, new, flow = item
    old = old if o["chunks"] == 2 else None
    kw = dict(norm=o["norm"], per_sample=o["per_sample"], spike_th=o["spike_th"], mask_events=o["mask_events"])
    got, rows = run_kernel(old, new, flow, crop, params, want_event_mask=o["want_event_mask"], **kw)
    want = M.augment_resize(L.DenseSparseAugmentor(list(crop)), old, new, flow, params, **kw)
    assert same_bits(got["out"], want["out"]), ("out", o, params)
    assert M.same_bits_or_nan(got["label"], want["label"]), ("label", o, params)
    assert same_bits(got["mask"], want["mask"]), ("mask", o, params)
    assert not o["want_event_mask"] or same_bits(got["event_mask"], want["event_mask"]), ("event_mask", o, params)
    return got, rows


def launches(rows):
    return [(short(r[0]), r[1], r[2]) for r in rows]


@pytest.mark.parametrize("idx", range(12))
@pytest.mark.parametrize("shape,crop", SHAPES)
def test_kernel_equals_the_numpy_restatement(shape, crop, idx):
    o, params = option_set(idx), make_params(idx, shape, crop)
    got, rows = check_against_restatement(make_item(shape, 100 + idx), crop, params, o)
    B, h, w = shape[0], *crop
    # the dispatch: min(ceil(h w / 256), max(1024 / B, 1)) workgroups of 256 per sample, then the finish kernel, a lane per pixel
    need, cap = -(-h * w // 256), max(1024 // B, 1)
    finish = o["norm"] or o["spike_th"] is not None or o["want_event_mask"] or o["mask_events"]
    assert launches(rows) == [("augment_resize_kernel", min(need, cap) * B, 256)] + [("prepare_finish_kernel", -(-B * h * w // 256), 256)] * bool(finish)
    if o["norm"] == "minmax" and o["spike_th"] is None:
        assert got["out"].max() == 1.0 and got["out"].min() == 0.0
    assert set(np.unique(got["mask"])) <= {0.0, 1.0} and np.isfinite(got["label"]).all()


def test_parameter_cases_cover_what_they_claim():
    seen = set()
    for shape, crop in SHAPES:
        for idx in range(12):
            for p in make_params(idx, shape, crop):
                top = (p.size[0] - crop[0], p.size[1] - crop[1])
                seen |= {("resized", p.resized), ("flips", p.hflip, p.vflip)}
                seen |= {("origin", "zero" if (p.y0, p.x0) == (0, 0) else "top")} if (p.y0, p.x0) in ((0, 0), top) else set()
                if p.resized:
                    seen |= {("x", p.scale_x < 1), ("y", p.scale_y < 1)}
            assert len({(p.resized, p.scale_x, p.hflip, p.y0) for p in make_params(idx, shape, crop)}) > 1 or idx < 4
    assert seen == {("resized", True), ("resized", False), ("origin", "zero"), ("origin", "top"), ("x", True), ("x", False), ("y", True),
                    ("y", False)} | {("flips", a, b) for a in (False, True) for b in (False, True)}
    assert {option_set(i)["chunks"] for i in range(12)} == {1, 2}


def test_batch_limit():
    """B = 64 runs - with more pixels per sample than its 16 workgroups cover in one trip - and B = 65 is refused."""
    shape, crop = (64, 2, 80, 90), (72, 64)
    params = make_params(7, shape, crop)
    o = dict(option_set(2), chunks=2)
    _, rows = check_against_restatement(make_item(shape, 700), crop, params, o)
    assert -(-crop[0] * crop[1] // 256) > 1024 // 64 and launches(rows)[0] == ("augment_resize_kernel", 16 * 64, 256)
    v, f = torch.zeros((65, 2, 21, 25), device=DEV), torch.zeros((65, 2, 21, 25), device=DEV)
    with pytest.raises(hip.SdfError) as e:
        hip.augment_resize_chunk(v, v, f, (8, 10), make_params(4, (65, 2, 21, 25), (8, 10)))
    assert e.value.rc == hip.E_SHAPE
    assert hip.lib().sdf_augment_resize_workspace_bytes(65) == 0


@pytest.mark.parametrize("kind", ["zero_sample", "equal"])
@pytest.mark.parametrize("shape,crop", SHAPES[:2])
def test_nothing_to_normalise(shape, crop, kind):
    """A sample that is all zero (per-sample min-max: its pair stays empty; its event mask is 0 everywhere) and volumes whose non-zeros
    are all +-0.75, copied without a resize (lo == hi: left unnormalised)."""
    for idx in (1, 2, 4, 8):                                       # min-max over the batch and per sample, with and without threshold
        o = dict(option_set(idx), want_event_mask=True)
        params = make_params(4 if kind == "equal" else idx, shape, crop)
        got, _ = check_against_restatement(make_item(shape, 300 + idx, kind), crop, params, o)
        if kind == "zero_sample":
            assert not got["out"][-1].any() and not got["event_mask"][-1].any()
            assert not o["mask_events"] or not got["mask"][-1].any()
        elif o["spike_th"] is None:
            assert set(np.unique(got["out"])) == {0.0, 0.75}
    # no norm, no threshold, no event mask: the gather alone
    old, new, flow = make_item(shape, 301, kind)
    params = make_params(0, shape, crop)
    got, rows = run_kernel(old, new, flow, crop, params, want_event_mask=False)
    assert [short(r[0]) for r in rows] == ["augment_resize_kernel"]
    assert same_bits(got["out"], M.augment_resize(L.DenseSparseAugmentor(list(crop)), old, new, flow, params)["out"])


@pytest.mark.parametrize("shape,crop", SHAPES[:2])
def test_flow_cases(shape, crop):
    """Flows with inf, -inf, NaN and exact zeros, resized (where an infinite tap at weight 0 gives NaN) and not, under every flip."""
    item = make_item(shape, 400, "flow_cases")
    seen = set()
    for idx in (0, 3, 4, 6, 9):
        got, _ = check_against_restatement(item, crop, make_params(idx, shape, crop), dict(option_set(idx), mask_events=False))
        lab, m = got["label"], got["mask"][:, 0]
        bad = ~np.isfinite(lab).all(axis=1)
        zero = (lab == 0).all(axis=1)
        assert not m[bad].any() and not m[zero].any() and m[~bad & ~zero].all()
        seen |= {name for name, there in (("inf", np.isinf(lab).any()), ("nan", np.isnan(lab).any()), ("zero", zero.any())) if there}
    assert seen == {"inf", "nan", "zero"}


def mdr_config(crop, chunks, norm, th, mask_events):
    return {"model": {"norm_input": norm, "encoding": "voxel"}, "loader": {"polarity": True, "crop": list(crop), "min_scale": -0.3, "max_scale": 0.5},
            "data": {"spike_th": th, "num_chunks": chunks}, "metrics": {"mask_events": mask_events}}


def check_against_torch(old, new, flow, cfg, params):
    aug = train.mdr_train_augmentor(cfg)
    sample = {"d_event_volume_old": old, "d_event_volume_new": new, "flow": flow}
    got = train.prepare_mdr_item(sample, cfg, aug, params)
    want = train.prepare_mdr_item_torch(sample, cfg, aug, params)
    torch.cuda.synchronize()
    for name, a, b in zip(("x", "label", "mask"), got, want):
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape, name
        assert same_bits(a, b), (name, params)                     # (both sides' NaNs are the GPU's: the flow too is compared strictly)
    return got


def test_equals_the_torch_composition_on_the_fixture_inputs():
    """Every record of the fixture as one batch over its inputs - the reference's own draws - against the torch sequence on the GPU."""
    rec = [M.params_of(r, L.ResizeParams) for r in GOLDEN["records"]]
    vols, flow = zip(*(M.fixture_inputs(k) for _, k in GOLDEN["seeds"].tolist()))
    old, new = (torch.from_numpy(np.stack([v[i] for v in vols]).transpose(0, 3, 1, 2).copy()).to(DEV) for i in (2, 3))
    fl = torch.from_numpy(np.stack(flow).transpose(0, 3, 1, 2).copy()).to(DEV)
    for n, (chunks, norm, th, me) in enumerate(((2, "minmax", None, True), (1, None, 0.5, False), (2, "minmax", 0.5, True), (1, "minmax", None, False))):
        x, lab, m = check_against_torch(old, new, fl, mdr_config(M.CROP, chunks, norm, th, me), rec)
        assert x.shape == (len(rec), 3 * chunks, 2, *M.CROP)
    # the volumes of one record against the reference's own item
    for b, (seed, _) in enumerate(GOLDEN["seeds"].tolist()):
        want = np.concatenate((GOLDEN[f"s{seed}_dimg1"], GOLDEN[f"s{seed}_dimg2"]), axis=2).transpose(2, 0, 1)
        x, lab, m = hip.augment_resize_chunk(old[b:b + 1], new[b:b + 1], fl[b:b + 1], M.CROP, rec[b], norm_input=None)
        assert same_bits(x[0, :, 0] - x[0, :, 1], want + np.float32(0)), seed                   # (pos - neg; a -0 of the reference is +0)
        assert M.same_bits_or_nan(lab[0].cpu().numpy(), GOLDEN[f"s{seed}_item_flow"]) and same_bits(m[0, 0], GOLDEN[f"s{seed}_valid"])


def test_equals_the_torch_composition_on_a_random_item():
    """Records drawn by the augmentor itself (numpy's generator under three seeds) at the middle shape, flows with inf / NaN among them."""
    shape, crop = SHAPES[1]
    old, new, flow = (torch.from_numpy(a).to(DEV) for a in make_item(shape, 500, "flow_cases"))
    seen = set()
    for seed, chunks, norm, th, me in ((0, 2, "minmax", None, True), (1, 1, "minmax", 0.5, False), (5, 2, None, None, True)):
        cfg = mdr_config(crop, chunks, norm, th, me)
        np.random.seed(seed)
        params = train.mdr_train_augmentor(cfg).sample_batch(shape[0], shape[2:])
        check_against_torch(old, new, flow, cfg, params)
        seen |= {p.resized for p in params}
        # drawn inside: the same records, the generator left where the augmentor leaves it
        np.random.seed(seed)
        again = train.prepare_mdr_item({"d_event_volume_old": old, "d_event_volume_new": new, "flow": flow}, cfg, train.mdr_train_augmentor(cfg))
        after = np.random.rand()
        np.random.seed(seed)
        train.mdr_train_augmentor(cfg).sample_batch(shape[0], shape[2:])
        assert after == np.random.rand()
        want = hip.augment_resize_chunk(old if chunks == 2 else None, new, flow, crop, params, norm_input=norm, spike_th=th, mask_events=me)
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(again, want))
    assert seen == {False, True}
    with pytest.raises(hip.SdfError) as e:                         # one row past the last origin
        bad = L.ResizeParams(False, 1.0, 1.0, tuple(shape[2:]), False, False, shape[2] - crop[0] + 1, 0)
        hip.augment_resize_chunk(old, new, flow, crop, bad)
    assert e.value.rc == hip.E_SHAPE
    with pytest.raises(hip.SdfError) as e:
        hip.augment_resize_chunk(old, new, flow, crop, params, norm_input="std")
    assert e.value.rc == hip.E_DTYPE
    with pytest.raises(hip.SdfError):
        hip.augment_resize_chunk(old, new, flow, crop, params[:-1])


def test_train_step_from_mdr_item():
    """The smallest model the training tests step (tests/test_train_gpu.py small_model: the en4 config's 3-encoder model at 144 x 144,
    batch 2) from a 150 x 156 MDR item of 2 x 5 bins: the prepared tensors are the torch sequence's, the loss is train_step's on them
    from a twin with the same initial state, and the front end is the library's launches alone - the clear of the min / max pairs (a
    memset, not in the kernel log), the gather and the finish - with no torch kernel: the only aten calls on the device are
    allocations."""
    from test_train_gpu import CFG, small_model
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    cfg = yaml.safe_load(open(CFG))
    cfg["loader"].update(crop=[144, 144], min_scale=-0.2, max_scale=0.5)
    cfg["data"]["num_chunks"] = 2
    cfg["metrics"]["mask_events"] = True
    assert cfg["model"]["norm_input"] == "minmax" and cfg["loader"]["polarity"] and cfg["data"]["spike_th"] is None
    sample = {"d_event_volume_old": synth_voxel(2, 5, 150, 156, seed=1234 + 5).to(DEV),
              "d_event_volume_new": synth_voxel(2, 5, 150, 156, seed=1234 + 6).to(DEV), "flow": synth_label(2, 150, 156)[0].to(DEV)}
    aug = train.mdr_train_augmentor(cfg)
    assert isinstance(aug, L.DenseSparseAugmentor) and aug.crop_size == [144, 144] and aug.do_flip

    np.random.seed(21)
    params = aug.sample_batch(2, (150, 156))
    assert any(p.resized for p in params)
    with AtenOps() as ops:
        x, lab, m = train.prepare_mdr_item(sample, cfg, aug, params)
    assert all(n.startswith("aten.empty") for n in ops.names), ops.names
    want = train.prepare_mdr_item_torch(sample, cfg, aug, params)
    assert x.shape == (2, 10, 2, 144, 144) and all(same_bits(a, b) for a, b in zip((x, lab, m), want))
    plain = train.prepare_mdr_item_torch(sample, {**cfg, "metrics": {**cfg["metrics"], "mask_events": False}}, aug, params)[2]
    assert 0 < float(m.sum()) < float(plain.sum())                  # mask_events took the pixels without an event away

    model, *_ = small_model()
    twin, *_ = small_model()
    opt, opt2 = (torch.optim.AdamW(mm.parameters(), lr=1e-4, weight_decay=0.01) for mm in (model, twin))
    np.random.seed(21)
    with hip.launch_log() as log:
        loss = train.train_step_from_mdr_item(model, opt, sample, cfg, aug)             # (draws the same records itself)
    loss2 = train.train_step(twin, opt2, *want)
    print(f"train_step_from_mdr_item loss {loss.item()!r}, train_step on the torch sequence's tensors {loss2.item()!r}")
    assert [short(r[0]) for r in log.rows[:2]] == ["augment_resize_kernel", "prepare_finish_kernel"] and len(log.rows) > 2
    assert "augment" not in " ".join(r[0] for r in log.rows[2:]) and "prepare_" not in " ".join(r[0] for r in log.rows[2:])
    assert torch.isfinite(loss) and loss.item() == loss2.item()
