"""The image of warped events and the Flow Warp Loss without a GPU: the definition's numpy restatement (tests/iwe_cases.py) on the
worked example, the zero flow and the moving dots; the new entry points' refusal codes with dummy pointers, before any launch; and
the loops' refusal of fwl=True on a voxel sample."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import iwe_cases as K
from test_abi_cpu import loaded_lib

f32 = np.float32
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4


def test_worked_example():
    """Window 4 x 8, one event x = 2, y = 1, tn = 0.25, p = 1, flow (4, -2) at its pixel, t_ref = 1: d = 0.75, xw = 5.0, yw = -0.5."""
    flow = np.zeros((2, 4, 8), dtype=f32)
    flow[0, 1, 2], flow[1, 1, 2] = 4.0, -2.0
    # (two far events of the other polarity give the list its time range; they land in channel 1)
    ev = dict(x=[7.0, 2.0, 7.0], y=[3.0, 1.0, 3.0], t=[0.0, 0.25, 1.0], p=[0.0, 1.0, 0.0])
    want = np.zeros((4, 8), dtype=f32)
    want[0, 5] = 0.5                                                           # the corner at y = -1 is dropped
    got = K.restate(ev["x"], ev["y"], ev["t"], ev["p"], flow)
    assert np.array_equal(got[0], want) and got[1].sum() == 2
    want[0, 5] = 1.0                                                           # rint(-0.5) = -0: row 0
    got = K.restate(ev["x"], ev["y"], ev["t"], ev["p"], flow, mode="nearest")
    assert np.array_equal(got[0], want) and got[1].sum() == 2


def test_zero_flow_nearest_is_the_bincount_of_the_lookup_pixels():
    ev, flow = K.moving_dots()
    h, w = K.DOTS_WINDOW
    got = K.restate(ev["x"], ev["y"], ev["t"], ev["p"], np.zeros_like(flow), mode="nearest")
    xi, yi = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    ch = np.where(ev["p"] > 0, 0, 1)
    want = np.bincount(((ch * h + yi) * w + xi)[inside], minlength=2 * h * w).reshape(2, h, w)
    assert inside.all() and np.array_equal(got, want.astype(f32))
    # ... and the sensor window cut out of a larger sensor: the same image at the shifted coordinates
    got = K.restate(ev["x"] + 5, ev["y"] + 3, ev["t"], ev["p"], np.zeros_like(flow), crop_origin=(3, 5), mode="nearest")
    assert np.array_equal(got, want.astype(f32))


def test_fwl_of_the_moving_dots():
    """True flow: the events of a dot fall on one pixel (FWL well above 1); zero flow: exactly 1; the negated flow smears them further."""
    ev, flow = K.moving_dots()
    true, zero, negated = (K.fwl(ev["x"], ev["y"], ev["t"], ev["p"], f) for f in (flow, np.zeros_like(flow), -flow))
    print("FWL true %.4f zero %.4f negated %.4f" % (true, zero, negated))
    assert true > 1.5
    assert zero == 1.0
    assert negated < 0.9
    # scale multiplies the flow: half the flow at scale 2 is the true flow
    assert K.fwl(ev["x"], ev["y"], ev["t"], ev["p"], flow * f32(0.5), scale=2.0) == true
    # no events: no variance, NaN
    e = np.zeros(0, dtype=f32)
    assert math.isnan(K.fwl(e, e, e, e, flow))


def iwe_desc(hip, **kw):
    d = hip.EventIweDesc()
    for f in ("x", "y", "t", "p", "flow", "keys", "keys_sorted", "order", "out", "workspace"):
        setattr(d, f, 0x10000)
    d.n_events, d.B, d.H, d.W, d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = 1000, 1, 40, 52, 32, 40, 3, 5
    d.workspace_bytes, d.scale, d.t_ref, d.win_a, d.win_b = 1 << 30, 1.0, 1.0, 0.0, 1.0
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def test_entry_points_refuse_before_any_launch():
    """Dummy pointers: every call returns from its host checks (no GPU here, and nothing may be launched on a refusal).  The last check
    of a call that passes all the others is the device-memory one: a host pointer is SDF_E_DTYPE."""
    from sdformerflow_amd import hip
    lib = loaded_lib()
    need = lib.sdf_event_iwe_workspace_bytes
    pad = lambda v: (v + 255) // 256 * 256
    assert need(1000, 1, 40, 52, 32, 40, 3, 5, 0) == 2 * pad(1000 * 8) + pad(2 * 33 * 41 * 8)  # records, sorted records, run table
    assert need(1000, 1, 40, 52, 32, 40, 3, 5, 1) == pad(2 * 33 * 41 * 8)                      # nearest: the run table alone
    assert need(1000, 1, 40, 52, 32, 40, 9, 5, 0) == 0 and need(1000, 1, 40, 52, 32, 0, 0, 0, 0) == 0 and need(1000, 1, 40, 52, 0, 0, 0, 0, 2) == 0
    assert need(-1, 1, 40, 52, 0, 0, 0, 0, 0) == 0 and need(1000, 0, 40, 52, 0, 0, 0, 0, 0) == 0
    for fn in (lib.sdf_event_iwe_keys_fwd, lib.sdf_event_iwe_gather_fwd):
        call = lambda **kw: fn(C.byref(iwe_desc(hip, **kw)), None)
        assert fn(None, None) == E_NULL
        assert call(crop_oy=9) == E_SHAPE                                      # the window leaves the sensor
        assert call(B=0) == E_SHAPE and call(n_events=-1) == E_SHAPE
        assert call(mode=2) == E_DTYPE and call(xy_dtype=3) == E_DTYPE
        assert call(win_a=0.5, win_b=0.5) == E_SHAPE and call(t_ref=math.inf) == E_SHAPE and call(scale=math.nan) == E_SHAPE
        assert call(flow=None) == E_NULL and call(out=None) == E_NULL and call(workspace=None) == E_NULL
        assert call(workspace_bytes=1000) == E_SHAPE
        assert call(workspace=0x10008) == E_ALIGN and call(out=0x10002) == E_ALIGN and call(flow=0x10001) == E_ALIGN
        assert call(B=2) == E_NULL                                             # several lists need their offsets
        offs = (C.c_int64 * 3)(0, 600, 900)
        assert call(B=2, offsets=C.addressof(offs)) == E_SHAPE                 # ... that end at n_events
        flat = (C.c_float * 2)(7.0, 7.0)
        assert call(t_range=C.addressof(flat)) == E_SHAPE                      # t_last == t_first
        assert call() == E_DTYPE                                               # everything in order but the memory: not the device's
    keys, gather = lib.sdf_event_iwe_keys_fwd, lib.sdf_event_iwe_gather_fwd
    assert keys(C.byref(iwe_desc(hip, p=None)), None) == E_NULL and keys(C.byref(iwe_desc(hip, keys=None)), None) == E_NULL
    assert keys(C.byref(iwe_desc(hip, xy_dtype=1)), None) == E_NULL            # integer coordinates without their map
    assert keys(C.byref(iwe_desc(hip, xy_dtype=1, rectify_map=0x10000)), None) == E_SHAPE
    assert keys(C.byref(iwe_desc(hip, rectify_map=0x10000)), None) == E_DTYPE
    assert keys(C.byref(iwe_desc(hip, x=0x10002)), None) == E_ALIGN and keys(C.byref(iwe_desc(hip, x=0x10002, y=0x10002, xy_dtype=2, rectify_map=0x10000, map_h=4, map_w=4)), None) == E_DTYPE
    assert keys(C.byref(iwe_desc(hip, n_events=0)), None) == 0                 # nothing to do, nothing touched
    assert gather(C.byref(iwe_desc(hip, order=None)), None) == E_NULL and gather(C.byref(iwe_desc(hip, order=0x10004)), None) == E_ALIGN

    def stats(**kw):
        d = hip.IweStatsDesc()
        d.iwe = d.table = d.workspace = 0x10000
        d.B, d.H, d.W, d.row0, d.rows, d.workspace_bytes = 2, 32, 40, 1, 3, 1 << 20
        for f, v in kw.items():
            setattr(d, f, v)
        return lib.sdf_iwe_stats_fwd(C.byref(d), None)
    assert lib.sdf_iwe_stats_workspace_bytes(2, 32, 40) == 2 * 2 * 4 * 8 and lib.sdf_iwe_stats_workspace_bytes(0, 32, 40) == 0
    assert lib.sdf_iwe_stats_fwd(None, None) == E_NULL and stats(iwe=None) == E_NULL and stats(table=None) == E_NULL
    assert stats(B=0) == E_SHAPE and stats(row0=2) == E_SHAPE and stats(row0=-1) == E_SHAPE and stats(workspace_bytes=64) == E_SHAPE
    assert stats(iwe=0x10002) == E_ALIGN and stats(table=0x10004) == E_ALIGN
    assert stats() == E_DTYPE


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.loss.flow_warp import FWL
    e = torch.zeros(4)
    with pytest.raises(hip.SdfError):
        hip.event_iwe(e, e, e, e, torch.zeros(1, 2, 4, 8), (4, 8))
    with pytest.raises(hip.SdfError):
        hip.iwe_stats(torch.zeros(1, 2, 4, 8))
    with pytest.raises(hip.SdfError):
        harness.warp_events({"x": e, "y": e, "t": e, "p": e}, torch.zeros(1, 2, 4, 8), (4, 8), None, 1.0)
    with pytest.raises(hip.SdfError):
        FWL(torch.zeros(1, 2, 4, 8), {"x": e, "y": e, "t": e, "p": e}, (4, 8), None, 1.0)()


def test_warp_times_normalises_float64_seconds_before_the_cast():
    from sdformerflow_amd import harness
    ts = torch.tensor([1.7e9 + k / 1024 for k in (0, 1, 2, 512, 1024)], dtype=torch.float64)
    got = harness.warp_times(ts)
    assert got.dtype == torch.float32 and got.tolist() == [0.0, 1 / 1024, 2 / 1024, 0.5, 1.0]
    assert len(set(ts.to(torch.float32).tolist())) == 1                      # (the cast alone loses them)
    assert harness.warp_times(torch.full((3,), 5.0, dtype=torch.float64)).tolist() == [0.0, 0.0, 0.0]
    ticks = torch.tensor([100, 150, 300], dtype=torch.int64)
    assert torch.equal(harness.warp_times(ticks), harness.event_times(ticks))


@pytest.mark.parametrize("loop", ["evaluate", "evaluate_mv"])
def test_fwl_on_a_voxel_sample_raises(loop):
    """The warp needs the event list: a sample that came as a voxel tensor is refused before anything is computed."""
    from sdformerflow_amd import harness
    cfg = {"loader": {"crop": None, "resolution": [4, 8]}, "metrics": {"flow_scaling": 1}, "model": {}, "data": {}}
    if loop == "evaluate":
        samples = [(torch.zeros(1, 10, 4, 8), torch.ones(1, 4, 8), torch.zeros(1, 2, 4, 8))]
    else:
        samples = [{"event_volume_old": torch.zeros(1, 5, 4, 8), "event_volume_new": torch.zeros(1, 5, 4, 8),
                    "flow": torch.zeros(1, 2, 4, 8), "valid": torch.ones(1, 4, 8)}]
    with pytest.raises(ValueError, match="needs the event list"):
        getattr(harness, loop)(torch.nn.Identity(), samples, cfg, device="cpu", fwl=True)
