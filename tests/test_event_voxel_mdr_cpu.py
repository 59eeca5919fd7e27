"""The MVSEC / MDR event front end, CPU side: the stated semantics of the reference's EventSequenceToVoxelGrid_Pytorch are pinned by a
plain in-order restatement that reproduces the stored reference outputs bit for bit; the fixture holds the cases the kernels depend on;
the C ABI has the new entry points and refuses bad arguments before any launch; CPU tensors are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "events_voxel_mdr.npz")
LISTS = ("a", "b", "c", "d", "e", "f")
f32 = np.float32


def restate(events, size, pol=True, t_scale=1e6, passes=(0, 1)):
    """EventSequence(timestamp_multiplier=t_scale, convert_to_relative=True) + EventSequenceToVoxelGrid_Pytorch(normalize=False)
    (reference MDR_dataloader/loader_utils.py:359-362, 470-564) restated in order: float64 times, multiply then divide, one rounding of
    dts to fp32; the left pass, then the right pass, one fp32 add per kept event in list order (np.add.at is unbuffered and
    sequential).  An event outside the sensor adds nothing and an empty list gives zeros (the documented differences).
    (N, 4) float64 [ts, x, y, p] in, (nb, H, W) or (nb, 2, H, W) fp32 out."""
    nb, H, W = size
    grids = [np.zeros(nb * H * W, dtype=f32) for _ in range(1 if pol else 2)]
    if len(events):
        ts = events[:, 0] * t_scale
        ts = ts - ts[0]
        delta = ts[-1] - ts[0]
        if delta == 0:
            delta = 1.0
        tn = (nb - 1) * (ts - ts[0]) / delta
        tis = np.floor(tn)
        dts = (tn - tis).astype(f32)
        xs, ys, ti = np.trunc(events[:, 1]).astype(np.int64), np.trunc(events[:, 2]).astype(np.int64), tis.astype(np.int64)
        pols = events[:, 3].astype(f32)
        pols[pols == 0] = -1
        inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        sels = [np.ones(len(events), bool)] if pol else [pols == 1, pols == -1]
        for shift, wt in [((0, f32(1.0) - dts), (1, dts))[k] for k in passes]:
            keep = inside & (tis >= 0) & (tis + shift < nb)
            index = xs + ys * W + (ti + shift) * W * H
            vals = pols * wt if pol else wt
            for g, sel in zip(grids, sels):
                np.add.at(g, index[keep & sel], vals[keep & sel])
    out = [g.reshape(nb, H, W) for g in grids]
    return out[0] if pol else np.stack(out, 1)


def normalise64(grid):
    """The reference's normalisation (:567-575) evaluated in float64 on fp32 grid bits; the result is float64."""
    g = grid.astype(np.float64)
    nz = g != 0
    if nz.any():
        mean = g[nz].mean()
        std = g[nz].std(ddof=1) if nz.sum() > 1 else float("nan")
        g[nz] = (g[nz] - mean) / std if std > 0 else g[nz] - mean
    return g


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def golden():
    return np.load(GOLDEN)


def golden_lists():
    z = golden()
    for name in LISTS:
        yield name, tuple(int(v) for v in z[name + "_size"]), z[name + "_events"], {k: z[f"{name}_{k}"] for k in ("raw", "norm", "pol", "poln")}


def measured_norm_error(form="signed"):
    """The largest absolute difference, over the fixture's lists, between the reference's normalised grid ("signed": the (nb, H, W)
    volumes; "polarities": the pol=False form) and a float64 evaluation of its formula on its own un-normalised bits: what fp32
    evaluation and torch's reduction order cost the reference itself."""
    raw, norm = ("raw", "norm") if form == "signed" else ("pol", "poln")
    return max(float(np.abs(ref[norm].astype(np.float64) - normalise64(ref[raw])).max()) for name, size, ev, ref in golden_lists())


def test_fixture_holds_the_cases_the_kernels_depend_on():
    z = golden()
    assert os.path.getsize(GOLDEN) < 512 * 1024
    cases = dict((name, (size, ev, ref)) for name, size, ev, ref in golden_lists())
    for name in ("a", "b"):
        (nb, H, W), ev, ref = cases[name]
        t = ev[:, 0]
        assert ev.dtype == np.float64 and t.min() > 1.4e9 and (np.diff(t) >= 0).all()
        steps = np.diff(t)[np.diff(t) > 0]
        assert steps.min() < 2e-6 and (np.diff(t) == 0).sum() > 1000                          # microsecond spacing, many equal stamps
        assert (t == t[-1]).sum() >= 5 and ref["raw"][nb - 1].any()                           # tis = nb - 1: the left pass only
        assert np.unique(t.astype(f32)).size == 1                                             # (what an fp32 time path would see)
        tn = (nb - 1) * (t * 1e6 - t[0] * 1e6) / (t[-1] * 1e6 - t[0] * 1e6)
        cells, counts = np.unique(np.stack((np.floor(tn), ev[:, 2], ev[:, 1])), axis=1, return_counts=True)
        assert np.sort(counts)[-2] >= 300                                                     # two hot pixels, each inside one bin
        assert (ref["raw"] < 0).any() and (ref["raw"] > 0).any()
    assert set(np.unique(cases["a"][1][:, 3])) == {0.0, 1.0} and set(np.unique(cases["b"][1][:, 3])) == {-1.0, 1.0}
    assert np.unique(cases["c"][1][:, 0]).size == 1 and len(cases["c"][1]) > 1 and not cases["c"][2]["raw"][1:].any()
    assert len(cases["d"][1]) == 0 and not cases["d"][2]["raw"].any() and len(cases["e"][1]) == 1
    assert cases["f"][0] == (10, 30, 40) and all(cases[n][0] == (5, 36, 44) for n in "abcde")
    assert z["ab_chunk"].shape == (1, 10, 2, 36, 44) and z["ab_event_mask"].shape == (1, 1, 36, 44)
    assert 0 < z["ab_event_mask"].sum() < 36 * 44


def test_in_order_restatement_reproduces_the_reference_bit_for_bit():
    """The contract of the HIP kernels: float64 times, the left pass then the right pass, list order inside a pass."""
    for name, size, ev, ref in golden_lists():
        assert np.array_equal(bits(restate(ev, size)), bits(ref["raw"])), name
        assert np.array_equal(bits(restate(ev, size, pol=False)), bits(ref["pol"])), name


def test_another_order_or_fp32_times_do_not_reproduce_it():
    """(The check above has teeth: the right pass before the left pass gives other bits on the hot cells, and so do fp32 times.)"""
    name, size, ev, ref = next(golden_lists())
    nb, H, W = size
    other = restate(ev, size, passes=(1, 0))
    assert np.allclose(other, ref["raw"], atol=1e-3) and not np.array_equal(bits(other), bits(ref["raw"]))
    ev32 = ev.copy()
    ev32[:, 0] = ev[:, 0].astype(f32)
    assert not np.array_equal(bits(restate(ev32, size)), bits(ref["raw"]))
    half = ev.copy()
    half[:, 0] = ev[0, 0] + (ev[:, 0] - ev[0, 0]).astype(f32).astype(np.float64)              # rounding AFTER the subtraction is harmless here,
    assert np.abs(restate(half, size) - ref["raw"]).max() < 1e-3                              # rounding the epoch stamps is not


def test_loop_restatement_matches_the_stored_chunk():
    """prepare_chunk on cat(old, new) is the loop's :162-213, and the mask is its :217-219 - on the reference's own volumes, exactly."""
    from sdformerflow_amd import harness
    z = golden()
    vol = torch.cat((torch.from_numpy(z["a_norm"])[None], torch.from_numpy(z["b_norm"])[None]), dim=1)
    chunk = harness.prepare_chunk(vol, "minmax", None, True)
    assert np.array_equal(bits(chunk), bits(z["ab_chunk"]))
    assert np.array_equal(chunk.sum(1).sum(1, keepdim=True).bool().numpy(), z["ab_event_mask"])


def test_header_and_binding_have_the_new_entry_points():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in ("sdf_event_voxel_tb_workspace_bytes", "sdf_event_voxel_tb_keys_fwd", "sdf_event_voxel_tb_gather_fwd"):
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    assert "typedef struct SdfEventVoxelTbDesc" in hdr and issubclass(hip.EventVoxelTbDesc, C.Structure)
    assert callable(hip.event_voxel_tb)


def _desc(hip, keep, **kw):
    d = hip.EventVoxelTbDesc()
    d.x = d.y = d.t = d.p = d.keys = d.keys_sorted = d.order = d.out = d.workspace = 0x10000
    offs = (C.c_int64 * 3)(0, 400, 1000)
    keep.append(offs)
    d.offsets = C.addressof(offs)
    d.n_events, d.n_lists, d.lists_per_sample, d.nb, d.H, d.W, d.workspace_bytes = 1000, 2, 2, 10, 260, 346, 1 << 40
    d.mode = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_are_reported_before_any_launch():
    """Negative return = refused before any launch: these calls never touch the dummy pointers and need no GPU."""
    from sdformerflow_amd import hip
    from test_abi_cpu import loaded_lib
    lib = loaded_lib()
    E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
    keep = []
    for call in (lib.sdf_event_voxel_tb_keys_fwd, lib.sdf_event_voxel_tb_gather_fwd):
        assert call(None, None) == E_NULL
        assert call(C.byref(_desc(hip, keep, nb=0)), None) == E_SHAPE
        assert call(C.byref(_desc(hip, keep, crop_h=300, crop_w=256)), None) == E_SHAPE          # crop larger than the sensor
        assert call(C.byref(_desc(hip, keep, crop_h=256)), None) == E_SHAPE                      # half a crop
        assert call(C.byref(_desc(hip, keep, crop_h=256, crop_w=256, crop_oy=5, crop_ox=45)), None) == E_SHAPE   # 5 + 256 > 260
        assert call(C.byref(_desc(hip, keep, crop_h=256, crop_w=256, crop_oy=2, crop_ox=-1)), None) == E_SHAPE
        assert call(C.byref(_desc(hip, keep, crop_oy=2)), None) == E_SHAPE                       # an origin without a crop
        assert call(C.byref(_desc(hip, keep, mode=3)), None) == E_DTYPE
        assert call(C.byref(_desc(hip, keep, mode=0, lists_per_sample=1, norm=1)), None) == E_DTYPE      # min-max belongs to the split mode
        assert call(C.byref(_desc(hip, keep, mode=2, lists_per_sample=1, use_spike_th=1)), None) == E_DTYPE
        assert call(C.byref(_desc(hip, keep, mode=0, lists_per_sample=1, event_mask=0x10000)), None) == E_DTYPE
        assert call(C.byref(_desc(hip, keep, mode=0)), None) == E_DTYPE                          # paired lists outside the split mode
        assert call(C.byref(_desc(hip, keep, n_lists=1)), None) == E_SHAPE                       # one list is half a pair
        assert call(C.byref(_desc(hip, keep, offsets=None)), None) == E_NULL
        bad = (C.c_int64 * 3)(0, 1200, 1000)                                                     # offsets not ascending
        assert call(C.byref(_desc(hip, keep, offsets=C.addressof(bad))), None) == E_SHAPE
        bad = (C.c_int64 * 3)(0, 600, 900)                                                       # lists must cover the arrays
        assert call(C.byref(_desc(hip, keep, offsets=C.addressof(bad))), None) == E_SHAPE
        assert call(C.byref(_desc(hip, keep, workspace_bytes=4096)), None) == E_SHAPE            # smaller than the workspace query
        assert call(C.byref(_desc(hip, keep, workspace=0x10004)), None) == E_ALIGN
        assert call(C.byref(_desc(hip, keep, out=None)), None) == E_NULL
    keys, gather = lib.sdf_event_voxel_tb_keys_fwd, lib.sdf_event_voxel_tb_gather_fwd
    assert keys(C.byref(_desc(hip, keep, x=None)), None) == E_NULL
    assert keys(C.byref(_desc(hip, keep, t=0x10004)), None) == E_ALIGN                           # float64 times
    assert keys(C.byref(_desc(hip, keep, xy_dtype=3)), None) == E_DTYPE
    assert gather(C.byref(_desc(hip, keep, order=None)), None) == E_NULL
    assert gather(C.byref(_desc(hip, keep, order=0x10004)), None) == E_ALIGN
    q = lib.sdf_event_voxel_tb_workspace_bytes
    pad = lambda v: (v + 255) // 256 * 256
    # records | sorted records | run table | min / max ... and with normalize the whole grid is computed and its partial sums kept
    assert q(1000, 2, 10, 260, 346, 256, 256, 2, 45, 0) == 2 * pad(8000) + pad(2 * 10 * 256 * 256 * 8) + pad(2 * 16) + 256
    blocks = (10 * 260 * 346 + 255) // 256
    assert q(1000, 2, 10, 260, 346, 256, 256, 2, 45, 1) == 2 * pad(8000) + pad(2 * 10 * 260 * 346 * 8) + pad(2 * blocks * 24) + pad(2 * 16) + 256
    assert q(1000, 2, 10, 260, 346, 256, 256, 5, 45, 0) == 0 and q(1000, 2, 10, 260, 346, 300, 256, 0, 0, 0) == 0      # refused geometries
    assert q(-1, 2, 10, 260, 346, 0, 0, 0, 0, 0) == 0 and q(1000, 2000, 10, 480, 640, 0, 0, 0, 0, 0) == 0              # 31-bit keys


def test_cpu_tensors_are_refused():
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.MDR_dataloader.loader_utils import EventSequence, EventSequenceToVoxelGrid_Pytorch
    ev = torch.from_numpy(golden()["a_events"])
    cols = {"ts": ev[:, 0], "x": ev[:, 1].float(), "y": ev[:, 2].float(), "p": ev[:, 3].float()}
    with pytest.raises(hip.SdfError):
        hip.event_voxel_tb(cols["x"], cols["y"], cols["ts"], cols["p"], 5, (36, 44), t_scale=1e6)
    with pytest.raises(hip.SdfError):
        EventSequenceToVoxelGrid_Pytorch(5, gpu=True)(EventSequence(None, {"height": 36, "width": 44}, features=ev, timestamp_multiplier=1e6,
                                                                    convert_to_relative=True))
    with pytest.raises(hip.SdfError):
        harness.event_pairs_to_chunk((cols, cols), 5, (36, 44), None, "minmax", None)
