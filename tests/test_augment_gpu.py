"""hip.augment_chunk (csrc/prepare_chunk.hip, sdf_augment_chunk_fwd) on the GPU: bit for bit against its numpy restatement
(tests/augment_cases.py) and against the torch composition (the transforms of DSEC_dataloader.data_augmentation, harness.prepare_chunk,
mask * event_mask); the Philox field's reproducibility; and train.train_step_from_item beside train.train_step.

Every buffer a call touches is a window between guard bytes, checked after the call."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest
import torch
import yaml
from torch.utils._python_dispatch import TorchDispatchMode

from sdformerflow_amd import hip, train
from sdformerflow_amd.DSEC_dataloader import data_augmentation as D

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_cases as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A
# (B, bins, Hs, Ws), crop: less than one workgroup per sample | several | more cells per sample than the launch's grid covers in one trip
SHAPES = (((2, 3, 11, 13), (8, 10)), ((3, 5, 37, 41), (32, 36)), ((3, 5, 140, 140), (136, 136)))
GOLDEN = np.load(os.path.join(HERE, "golden", "augment.npz"))


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def kname(logged):
    m = re.search(r"(\w+)(?:<.*?>)?\(", logged)
    return m.group(1) if m else logged


class Guarded:
    """A window of `nbytes` with 256 guard bytes before and behind it, 256-byte aligned."""

    def __init__(self, nbytes, fill=None):
        self.nbytes = nbytes
        self.outer = torch.full((nbytes + 1024,), GUARD, dtype=torch.uint8, device=DEV)
        self.off = 256 + (-(self.outer.data_ptr() + 256)) % 256
        if fill is not None:
            self.window()[:] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(DEV)

    def window(self):
        return self.outer[self.off:self.off + self.nbytes]

    def ptr(self):
        return self.outer.data_ptr() + self.off

    def intact(self):
        return bool((self.outer[:self.off] == GUARD).all()) and bool((self.outer[self.off + self.nbytes:] == GUARD).all())

    def array(self, dtype, shape):
        return self.window().cpu().numpy().view(dtype).reshape(shape).copy()


def run_kernel(vox, label, valid, crop, origins, flips, drop_q, drop_u=None, seed=0, offset=0, norm=None, per_sample=False, spike_th=None,
               mask_events=False, want_event_mask=True):
    """sdf_augment_chunk_fwd called directly on numpy inputs, every buffer a guarded window.  Returns the outputs as numpy arrays and the
    launch log's rows."""
    B, bins, Hs, Ws = vox.shape
    h, w = crop if crop else (Hs, Ws)
    lib = hip.lib()
    ws_bytes = lib.sdf_augment_chunk_workspace_bytes(B)
    assert ws_bytes == 8 * B
    bufs = {"voxel": Guarded(vox.nbytes, vox), "out": Guarded(B * bins * 2 * h * w * 4), "workspace": Guarded(ws_bytes)}
    if label is not None:
        bufs["label"], bufs["label_out"] = Guarded(label.nbytes, label), Guarded(B * 2 * h * w * 4)
    if valid is not None:
        bufs["valid"], bufs["mask_out"] = Guarded(valid.nbytes, valid), Guarded(B * h * w * 4)
    if drop_u is not None:
        bufs["drop_u"] = Guarded(drop_u.nbytes, drop_u)
    if want_event_mask:
        bufs["event_mask"] = Guarded(B * h * w * 4)
    d = hip.AugmentChunkDesc()
    for name, g in bufs.items():
        setattr(d, name, g.ptr())
    d.workspace_bytes, d.seed, d.offset = ws_bytes, seed, offset
    d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w = B, bins, Hs, Ws, (h if crop else 0), (w if crop else 0)
    d.valid_is_u8 = int(valid is not None and valid.dtype == np.uint8)
    d.norm, d.per_sample = int(norm == "minmax"), int(per_sample)
    d.use_spike_th, d.spike_th, d.mask_events = int(spike_th is not None), float(spike_th or 0.0), int(mask_events)
    for b in range(64):                                            # (entries beyond B are not looked at)
        d.oy[b], d.ox[b], d.flags[b], d.drop_q[b] = (*origins[b], flips[b], drop_q[b]) if b < B else (-9, 1 << 20, 255, 0.5)
    with hip.launch_log() as log:
        rc = lib.sdf_augment_chunk_fwd(C.byref(d), hip._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    broken = [name for name, g in bufs.items() if not g.intact()]
    assert not broken, f"a store outside {broken}"
    got = {"out": bufs["out"].array(np.float32, (B, bins, 2, h, w)),
           "label": bufs["label_out"].array(np.float32, (B, 2, h, w)) if label is not None else None,
           "mask": bufs["mask_out"].array(np.float32, (B, 1, h, w)) if valid is not None else None,
           "event_mask": bufs["event_mask"].array(np.float32, (B, 1, h, w)) if want_event_mask else None}
    for name, src in (("voxel", vox), ("label", label), ("valid", valid), ("drop_u", drop_u)):           # the inputs are left as they were
        assert src is None or np.array_equal(bufs[name].array(np.uint8, (-1,)), np.ascontiguousarray(src).view(np.uint8).reshape(-1)), name
    return got, log.rows


def make_item(shape, seed, kind="random"):
    """Signed voxel with ~40 % zeros (negative zeros among them) and per-sample ranges, a flow with some zeros, a valid map with values
    0, 1 and 2.5 (non-zero counts as valid)."""
    B, bins, Hs, Ws = shape
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.uniform(-1.0, 1.0, shape) * (1.0 + g.exponential(0.5, shape))
    v = np.where(g.random(shape) < 0.6, v, np.where(g.random(shape) < 0.5, 0.0, -0.0)) * (1.0 + np.arange(B)).reshape(B, 1, 1, 1)
    if kind == "zero_sample":                                      # one sample without an event
        v[B - 1] = 0.0
    if kind == "equal":                                            # every non-zero is +-0.75: lo == hi, left unnormalised
        v = np.where(v != 0.0, np.sign(v) * 0.75, 0.0)
    label = np.where(g.random((B, 2, Hs, Ws)) < 0.9, g.normal(0.0, 5.0, (B, 2, Hs, Ws)), 0.0)
    valid = g.choice(np.array([0.0, 1.0, 2.5]), size=(B, 1, Hs, Ws), p=[0.3, 0.6, 0.1])
    return v.astype(np.float32), label.astype(np.float32), valid.astype(np.float32)


def option_set(idx, shape, crop):
    """Case `idx` of 12 over one shape.  Together: all four flip words for every sample alike (0-3) and mixed per sample; the origins
    (0, 0), (Hs - h, Ws - w) and an interior one; no crop (5, 10); drop_q from {none, 0, 0.3, 1} rotating over the samples, a given
    field and Philox; norm none / whole batch / per sample; spike_th none / 0.5; mask_events; valid as fp32 and as bytes."""
    B, _, Hs, Ws = shape
    use_crop = idx not in (5, 10)
    h, w = crop if use_crop else (Hs, Ws)
    corners = [(0, 0), (Hs - h, Ws - w), ((Hs - h) // 2, (Ws - w + 1) // 2)]
    qs = [-1.0, 0.0, 0.3, 1.0]
    return dict(crop=crop if use_crop else None,
                origins=[corners[(b + idx) % 3] for b in range(B)],
                flips=[idx if idx < 4 else (b + idx) % 4 for b in range(B)],
                drop_q=[qs[(b + idx) % 4] for b in range(B)],
                given_u=(idx // 4) % 2 == 0,
                norm=[None, "minmax", "minmax"][idx % 3], per_sample=idx % 3 == 2,
                spike_th=[None, 0.5][idx % 2], mask_events=bool((idx // 2) % 2), valid_u8=bool((idx // 3) % 2))


def check_against_restatement(item, o, seed=0, offset=0):
    vox, label, valid = item
    B, bins = vox.shape[:2]
    h, w = o["crop"] if o["crop"] else vox.shape[2:]
    if o["valid_u8"]:
        valid = (valid != 0).astype(np.uint8)
    u = None
    if o["given_u"]:
        u = np.random.Generator(np.random.PCG64(77)).random((B, bins, h, w), dtype=np.float32)
        u.reshape(-1)[:3] = [0.0, 0.3, np.float32(0.3) + np.float32(2.0 ** -25)]                 # at and beside a q (fp32 comparison)
    kw = dict(drop_u=u, seed=seed, offset=offset, norm=o["norm"], per_sample=o["per_sample"], spike_th=o["spike_th"],
              mask_events=o["mask_events"])
    got, rows = run_kernel(vox, label, valid, o["crop"], o["origins"], o["flips"], o["drop_q"], **kw)
    want = A.augment(vox, label, valid, o["crop"], o["origins"], o["flips"], o["drop_q"], **kw)
    for k in ("out", "label", "mask", "event_mask"):
        assert same_bits(got[k], want[k]), (k, o)
    return got, rows


@pytest.mark.parametrize("idx", range(12))
@pytest.mark.parametrize("shape,crop", SHAPES)
def test_kernel_equals_the_numpy_restatement(shape, crop, idx):
    o = option_set(idx, shape, crop)
    got, rows = check_against_restatement(make_item(shape, 100 + idx), o, seed=0x1234567887654321 + idx, offset=(idx << 33) + 5)
    B, bins, Hs, Ws = shape
    h, w = o["crop"] if o["crop"] else (Hs, Ws)
    # the dispatch (sdf_augment_chunk_fwd): min(ceil(cells / 256), max(1024 / B, 1)) workgroups of 256 per sample, then the finish
    # kernel (the event mask is asked for here), a lane per pixel
    cells = bins * h * w
    need, cap = -(-cells // 256), max(1024 // B, 1)
    assert [kname(r[0]) for r in rows] == ["augment_split_kernel", "prepare_finish_kernel"], rows
    assert (rows[0][1], rows[0][2]) == (min(need, cap) * B, 256) and (rows[1][1], rows[1][2]) == (-(-B * h * w // 256), 256)
    if shape == SHAPES[2][0]:
        assert need > cap                                         # the stride loop takes a second trip
    if shape == SHAPES[0][0] and o["crop"]:
        assert cells < 256                                        # less than one workgroup
    if o["norm"] == "minmax" and o["spike_th"] is None:
        assert got["out"].max() == 1.0 and got["out"].min() == 0.0
    assert set(np.unique(got["mask"])) <= {0.0, 1.0} and set(np.unique(got["event_mask"])) <= {0.0, 1.0}


@pytest.mark.parametrize("kind", ["zero_sample", "equal"])
@pytest.mark.parametrize("shape,crop", SHAPES[:2])
def test_nothing_to_normalise(shape, crop, kind):
    """A sample that is all zero (per-sample min-max: its pair stays empty; its event mask is 0 everywhere) and a volume whose non-zeros
    are all +-0.75 (lo == hi: left unnormalised), dropped and not."""
    for idx in (1, 2, 4, 8):                                       # min-max over the batch and per sample, with and without threshold
        o = option_set(idx, shape, crop)
        got, _ = check_against_restatement(make_item(shape, 300 + idx, kind), o, seed=9, offset=idx)
        if kind == "zero_sample":
            assert not got["out"][-1].any() and not got["event_mask"][-1].any()
            assert not o["mask_events"] or not got["mask"][-1].any()
        elif o["spike_th"] is None:
            assert set(np.unique(got["out"])) == {0.0, 0.75}
    # no output asked for but the input: one launch without norm and threshold
    vox, _, _ = make_item(shape, 301, kind)
    B = shape[0]
    got, rows = run_kernel(vox, None, None, crop, [(1, 1)] * B, [3] * B, [-1.0] * B, want_event_mask=False)
    assert [kname(r[0]) for r in rows] == ["augment_split_kernel"]
    assert same_bits(got["out"], A.augment(vox, None, None, crop, [(1, 1)] * B, [3] * B, [-1.0] * B)["out"])


def torch_composition(v, label, mask, transform, drop_u, norm, th, mask_events):
    cfg = {"model": {"norm_input": norm, "encoding": "voxel"}, "loader": {"polarity": True}, "data": {"spike_th": th},
           "metrics": {"mask_events": mask_events}}
    return train.prepare_train_item_torch(v, label, mask, cfg, transform, drop_u)


def seeded(seed):
    random.seed(seed)
    torch.manual_seed(seed)


def check_against_torch(v, label, mask, transform, seed, u, norm, th, mask_events):
    B = v.shape[0]
    seeded(seed)
    p = transform.sample(v.shape)
    origins, flips, qs = p.per_sample(B)
    crop = None if tuple(p.crop) == tuple(v.shape[-2:]) else p.crop
    out_g, lab_g, mask_g, em_g = (Guarded(4 * n) for n in (v.shape[1] * 2 * B * p.crop[0] * p.crop[1], 2 * B * p.crop[0] * p.crop[1],
                                                           B * p.crop[0] * p.crop[1], B * p.crop[0] * p.crop[1]))
    carve = lambda g, shape: g.window().view(torch.float32).view(shape)
    h, w = p.crop
    em = carve(em_g, (B, 1, h, w))
    got = hip.augment_chunk(v, label, mask, crop, origins, flips, drop_q=qs, drop_u=u, norm_input=norm, spike_th=th, mask_events=mask_events,
                            out=carve(out_g, (B, v.shape[1], 2, h, w)), label_out=carve(lab_g, (B, 2, h, w)),
                            mask_out=carve(mask_g, (B, 1, h, w)), event_mask=em)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (out_g, lab_g, mask_g, em_g))
    seeded(seed)
    want = torch_composition(v, label, mask, transform, u, norm, th, mask_events)
    for name, a, b in zip(("x", "label", "mask"), got, want):
        assert a.dtype == b.dtype == torch.float32 and same_bits(a, b), (name, seed, p)
    assert torch.equal(em, want[0].sum(1).sum(1, keepdim=True).bool().float())
    return p


def test_equals_the_torch_composition_on_the_fixture_inputs():
    """Every case of the fixture - every accepted chain, under the seeds that show both outcomes of its coins - through the new
    transforms, harness.prepare_chunk and the event-mask product on the GPU, the recorded uniform field given to both sides."""
    names = A.chain_names()
    for n, (ci, seed, k, *_) in enumerate(GOLDEN["cases"].tolist()):
        v, label, mask = (torch.from_numpy(GOLDEN[f"in{k}_{name}"].astype(np.float32)).to(DEV) for name in ("voxel", "flow", "mask"))
        tag = f"c{ci}_s{seed}_u"
        u = torch.from_numpy(GOLDEN[tag]).to(DEV) if tag in GOLDEN else None
        p = check_against_torch(v, label, mask, A.build_chain(D, names[ci]), seed, u, [None, "minmax"][n % 2], [None, 0.5][(n // 2) % 2],
                                bool((n // 4) % 2))
        assert (p.drop_q is not None) == (u is not None)


@pytest.mark.parametrize("shape,crop", SHAPES)
def test_equals_the_torch_composition_on_a_random_input(shape, crop):
    """RandomCrop, both flips and a certain drop under three seeds, a uniform field drawn on the GPU given to both sides."""
    vox, label, valid = (torch.from_numpy(a).to(DEV) for a in make_item(shape, 500))
    valid = (valid != 0).float()                                   # (a transform chain without a flip hands the mask through as it is)
    B, bins = shape[:2]
    u = torch.rand((B, bins) + crop, generator=torch.Generator(DEV).manual_seed(1), device=DEV)
    flags = set()
    for seed, norm, th, me in ((0, "minmax", None, True), (1, "minmax", 0.5, False), (5, None, None, True)):
        t = D.Compose([D.RandomCrop(crop), D.Random_vertical_flip(0.5), D.Random_horizontal_flip(0.5), D.Random_event_drop(0.1, 0.6, p=1.0)])
        p = check_against_torch(vox, label, valid, t, seed, u, norm, th, me)
        assert p.drop_q is not None and 0.1 <= p.drop_q <= 0.6
        flags.add(p.flags)
    # byte masks and a (B, H, W) mask through the wrapper; its own buffers
    t = D.Compose([D.CenterCrop(crop), D.Random_horizontal_flip(1.0)])
    seeded(3)
    p = t.sample(shape)
    a = hip.augment_chunk(vox, label, valid, crop, p.origin, p.flags)
    b = hip.augment_chunk(vox, label, valid.bool().reshape(B, *shape[2:]), crop, *p.per_sample(B)[:2])
    assert p.flags == 1 and all(same_bits(x, y) for x, y in zip(a, b))
    seeded(3)
    assert all(same_bits(x, y) for x, y in zip(a, torch_composition(vox, label, valid, t, None, "minmax", None, False)))


def test_philox_field_is_reproducible_and_moves_with_the_offset():
    shape, crop = SHAPES[1]
    vox, label, valid = (torch.from_numpy(a).to(DEV) for a in make_item(shape, 600))
    B = shape[0]
    call = lambda seed, offset: hip.augment_chunk(vox, label, valid, crop, (2, 3), [0, 1, 2], drop_q=0.4, seed=seed, offset=offset)
    a, b, c, d = call(11, 7), call(11, 7), call(11, 8), call(12, 7)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], d[0]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    kept = float((a[0] != 0).sum()) / float((hip.augment_chunk(vox, None, None, crop, (2, 3), [0, 1, 2])[0] != 0).sum())
    assert 0.55 < kept < 0.65                                       # q = 0.4 over ~ 10 000 events: 0.6 +- 5 sigma
    with pytest.raises(hip.SdfError) as e:
        hip.augment_chunk(vox, label, valid, crop, (6, 3), 0)      # one row past the last origin
    assert e.value.rc == hip.E_SHAPE
    with pytest.raises(hip.SdfError) as e:
        hip.augment_chunk(vox, label, valid, crop, (0, 0), 0, norm_input="std")
    assert e.value.rc == hip.E_DTYPE
    with pytest.raises(hip.SdfError):
        hip.augment_chunk(vox, label, valid, crop, [(0, 0)] * (B - 1), 0)


class AtenOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        on_gpu = any(isinstance(a, torch.Tensor) and a.is_cuda for a in args) or "cuda" in str(kwargs.get("device"))
        if on_gpu:                                                 # (the transform's coins are CPU draws)
            self.names.append(str(func))
        return func(*args, **kwargs)


def test_train_step_from_item():
    """The smallest model the training tests step (tests/test_train_gpu.py small_model: the en4 config's 3-encoder model at 144 x 144,
    batch 2) from a 150 x 156 loader item: the prepared tensors are the torch composition's, the loss is train_step's on them from a
    twin with the same initial state, and the front end is the library's launches alone - the clear of the min / max pairs (a memset,
    not in the kernel log), the gather and the finish - with no torch kernel: the only aten calls on the device are allocations."""
    from test_train_gpu import CFG, small_model
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    cfg = yaml.safe_load(open(CFG))
    cfg["loader"]["crop"] = [144, 144]
    cfg["metrics"]["mask_events"] = True
    assert cfg["model"]["norm_input"] == "minmax" and cfg["loader"]["polarity"] and cfg["data"]["spike_th"] is None
    vox = synth_voxel(2, 10, 150, 156, seed=1234 + 4).to(DEV)
    label, mask = (t.to(DEV) for t in synth_label(2, 150, 156))
    t = train.train_transform(cfg)
    assert [type(a) for a in t.transforms] == [D.RandomCrop, D.Random_horizontal_flip, D.Random_vertical_flip] and t.transforms[0].size == (144, 144)

    seeded(21)
    with AtenOps() as ops:
        x, lab, m = train.prepare_train_item(vox, label, mask, cfg, t, step=3)
    assert all(n.startswith("aten.empty") for n in ops.names), ops.names
    seeded(21)
    want = train.prepare_train_item_torch(vox, label, mask, cfg, t)
    assert x.shape == (2, 10, 2, 144, 144) and all(same_bits(a, b) for a, b in zip((x, lab, m), want))
    seeded(21)
    plain = train.prepare_train_item_torch(vox, label, mask, {**cfg, "metrics": {**cfg["metrics"], "mask_events": False}}, t)[2]
    assert 0 < float(m.sum()) < float(plain.sum())                  # mask_events took the pixels without an event away

    model, *_ = small_model()
    twin, *_ = small_model()
    opt, opt2 = (torch.optim.AdamW(mm.parameters(), lr=1e-4, weight_decay=0.01) for mm in (model, twin))
    seeded(21)
    with hip.launch_log() as log:
        loss = train.train_step_from_item(model, opt, (vox, label, mask), cfg, t, step=3)
    loss2 = train.train_step(twin, opt2, *want)
    print(f"train_step_from_item loss {loss.item()!r}, train_step on the torch composition's tensors {loss2.item()!r}")
    assert [kname(r[0]) for r in log.rows[:2]] == ["augment_split_kernel", "prepare_finish_kernel"] and len(log.rows) > 2
    assert "augment" not in " ".join(r[0] for r in log.rows[2:]) and "prepare_" not in " ".join(r[0] for r in log.rows[2:])
    assert torch.isfinite(loss) and loss.item() == loss2.item()
