"""The event front end, CPU side: the accumulation order of the reference's VoxelGrid is pinned by a plain in-order restatement that
reproduces the stored reference outputs bit for bit; the C ABI refuses bad arguments before any launch; CPU tensors are refused."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "events_voxel.npz")
f32 = np.float32


def restate(x, y, t, p, size, polarities=False):
    """VoxelGrid.convert_CHW / convert_CHW_polarities (reference DSEC_dataloader/event_representations.py:248-313) restated in order:
    the eight corner passes x outer, y middle, t inner; inside a pass one fp32 add per kept event, in list order (np.add.at is
    unbuffered and sequential).  Every product is a separately rounded fp32 operation.  numpy fp32 arrays in, (C, H, W) or
    (C, 2, H, W) out."""
    Cb, H, W = size
    x, y, t, p = (np.ascontiguousarray(a, dtype=f32) for a in (x, y, t, p))
    grids = [np.zeros(Cb * H * W, dtype=f32) for _ in range(2 if polarities else 1)]
    if t.size == 0:
        out = [g.reshape(Cb, H, W) for g in grids]
        return np.stack(out, 1) if polarities else out[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        tn = (f32(Cb - 1) * (t - t[0])) / (t[-1] - t[0])
    x0, y0, t0 = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64), np.trunc(tn).astype(np.int64)
    value = f32(2) * p - f32(1)
    for xl in (x0, x0 + 1):
        for yl in (y0, y0 + 1):
            for tl in (t0, t0 + 1):
                keep = (xl < W) & (xl >= 0) & (yl < H) & (yl >= 0) & (tl >= 0) & (tl < Cb)
                wx, wy, wt = f32(1) - np.abs(xl.astype(f32) - x), f32(1) - np.abs(yl.astype(f32) - y), f32(1) - np.abs(tl.astype(f32) - tn)
                index = H * W * tl + W * yl + xl
                if polarities:
                    wgt = (wx * wy) * wt
                    for g, sel in zip(grids, (p == 1, p == 0)):
                        np.add.at(g, index[keep & sel], wgt[keep & sel])
                else:
                    wgt = ((value * wx) * wy) * wt
                    np.add.at(grids[0], index[keep], wgt[keep])
    out = [g.reshape(Cb, H, W) for g in grids]
    return np.stack(out, 1) if polarities else out[0]


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def golden_cases():
    z = np.load(GOLDEN)
    for name in ("a", "b"):
        yield name, tuple(int(v) for v in z[name + "_size"]), {k: z[f"{name}_{k}"] for k in "xytp"}, z[name + "_chw"], z[name + "_pol"]


def test_fixture_holds_the_cases_the_order_depends_on():
    for name, (Cb, H, W), ev, chw, pol in golden_cases():
        x, y, t, p = ev["x"], ev["y"], ev["t"], ev["p"]
        assert chw.shape == (Cb, H, W) and pol.shape == (Cb, 2, H, W) and chw.dtype == f32
        assert (np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() > 100                    # time order, equal timestamps
        assert ((x > -1) & (x < 0)).sum() >= 40 and ((y > -1) & (y < 0)).sum() >= 40
        assert (x >= W - 1).sum() >= 40 and (y >= H - 1).sum() >= 40 and (x < -2).sum() >= 20 and (y > H + 1).sum() >= 20
        assert (x != np.trunc(x)).sum() > 1000 and (x == np.trunc(x)).sum() > 300
        cells, counts = np.unique(np.stack((np.trunc(x), np.trunc(y))), axis=1, return_counts=True)
        assert counts.max() >= 600 and np.sort(counts)[-2] >= 300                           # hot pixels
        assert set(np.unique(p)) == {0.0, 1.0} and (t == t[-1]).sum() >= 5 and chw[Cb - 1].any()
        assert (chw < 0).any() and (chw > 0).any()


def test_in_order_restatement_reproduces_the_reference_bit_for_bit():
    """The contract of the HIP kernel: per cell, the corner passes in the reference's order and list order inside a pass."""
    for name, size, ev, chw, pol in golden_cases():
        got = restate(ev["x"], ev["y"], ev["t"], ev["p"], size)
        assert np.array_equal(bits(got), bits(chw)), name
        got = restate(ev["x"], ev["y"], ev["t"], ev["p"], size, polarities=True)
        assert np.array_equal(bits(got), bits(pol)), name


def test_another_order_does_not_reproduce_it():
    """(The check above has teeth: events summed in reversed list order give other bits on the hot cells.)"""
    name, size, ev, chw, _ = next(golden_cases())
    n = ev["t"].size
    idx = np.arange(n)
    idx[1:-1] = idx[1:-1][::-1]                  # the list reversed between its two ends: t[0], t[-1] and every event's t_norm stay
    other = restate(ev["x"][idx], ev["y"][idx], ev["t"][idx], ev["p"][idx], size)
    assert np.allclose(other, chw, atol=1e-3) and not np.array_equal(bits(other), bits(chw))


def _desc(hip, **kw):
    d = hip.EventVoxelDesc()
    d.x = d.y = d.t = d.p = d.keys = d.keys_sorted = d.order = d.out = d.workspace = 0x10000
    d.n_events, d.B, d.C, d.H, d.W, d.workspace_bytes = 1000, 1, 10, 480, 640, 1 << 40
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_are_reported_before_any_launch():
    """Negative return = refused before any launch: these calls never touch the dummy pointers and need no GPU."""
    from sdformerflow_amd import hip
    from test_abi_cpu import loaded_lib
    lib = loaded_lib()
    E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
    for call in (lib.sdf_event_voxel_keys_fwd, lib.sdf_event_voxel_gather_fwd):
        assert call(None, None) == E_NULL
        assert call(C.byref(_desc(hip, C=0)), None) == E_SHAPE
        assert call(C.byref(_desc(hip, crop_h=500, crop_w=600)), None) == E_SHAPE            # crop larger than the sensor
        assert call(C.byref(_desc(hip, crop_h=288)), None) == E_SHAPE                        # half a crop
        assert call(C.byref(_desc(hip, B=2)), None) == E_NULL                                # several lists need offsets
        assert call(C.byref(_desc(hip, mode=3)), None) == E_DTYPE
        assert call(C.byref(_desc(hip, norm=1)), None) == E_DTYPE                            # min-max belongs to the model-input form
        assert call(C.byref(_desc(hip, workspace_bytes=4096)), None) == E_SHAPE              # smaller than the workspace query
        assert call(C.byref(_desc(hip, workspace=0x10004)), None) == E_ALIGN
        assert call(C.byref(_desc(hip, out=None)), None) == E_NULL
        offs = (C.c_int64 * 3)(0, 600, 900)                                                  # lists must cover the arrays
        assert call(C.byref(_desc(hip, B=2, offsets=C.addressof(offs))), None) == E_SHAPE
        offs = (C.c_int64 * 3)(0, 400, 1000)
        rng = (C.c_float * 4)(0.0, 1.0, 5.0, 5.0)                                            # second list: first time == last time
        assert call(C.byref(_desc(hip, B=2, offsets=C.addressof(offs), t_range=C.addressof(rng))), None) == E_SHAPE
    keys, gather = lib.sdf_event_voxel_keys_fwd, lib.sdf_event_voxel_gather_fwd
    assert keys(C.byref(_desc(hip, x=None)), None) == E_NULL
    assert keys(C.byref(_desc(hip, xy_dtype=1)), None) == E_NULL                             # integer coordinates need the map
    assert keys(C.byref(_desc(hip, rectify_map=0x10000)), None) == E_DTYPE                   # fp32 coordinates are rectified already
    assert keys(C.byref(_desc(hip, t=0x10002)), None) == E_ALIGN
    assert gather(C.byref(_desc(hip, order=None)), None) == E_NULL
    assert gather(C.byref(_desc(hip, order=0x10004)), None) == E_ALIGN
    q = lib.sdf_event_voxel_workspace_bytes
    assert q(1000, 1, 10, 480, 640, 0, 0) == 2 * 16128 + ((11 * 481 * 641 * 8 + 255) // 256) * 256 + 256
    assert q(0, 1, 10, 480, 640, 288, 384) == ((11 * 289 * 385 * 8 + 255) // 256) * 256 + 256
    assert q(1000, 512, 20, 480, 640, 0, 0) == 0 and q(-1, 1, 10, 480, 640, 0, 0) == 0        # 31-bit keys; a negative count


def test_cpu_tensors_are_refused():
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.DSEC_dataloader.event_representations import VoxelGrid
    z = np.load(GOLDEN)
    ev = {k: torch.from_numpy(z[f"a_{k}"]) for k in "xytp"}
    with pytest.raises(hip.SdfError):
        hip.event_voxel(ev["x"], ev["y"], ev["t"], ev["p"], 5, (24, 32))
    with pytest.raises(hip.SdfError):
        VoxelGrid((5, 24, 32)).convert_CHW(ev)
    with pytest.raises(hip.SdfError):
        VoxelGrid((5, 24, 32)).convert_CHW_polarities(ev)
    with pytest.raises(hip.SdfError):
        harness.events_to_chunk(ev, 5, (24, 32), None, "minmax", None)
    config = {"loader": {"crop": None, "polarity": True, "resolution": [24, 32]}, "model": {"norm_input": "minmax", "num_bins": 5}, "data": {"spike_th": None},
              "metrics": {"flow_scaling": 1, "mask_events": False}}
    sample = ({"ts": ev["t"].long(), "x": ev["x"], "y": ev["y"], "p": ev["p"]}, torch.ones(24, 32), torch.zeros(2, 24, 32))
    with pytest.raises(hip.SdfError):                                                        # the event-dict path of evaluate, device "cpu"
        harness.evaluate(None, [sample], config, device="cpu")
