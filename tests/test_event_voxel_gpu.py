"""The event front end on the GPU (csrc/event_voxel.hip through hip.event_voxel, VoxelGrid, harness.events_to_chunk): every check is
bit for bit - the same fp32 operations in the same order give the same bits, so there is no tolerance anywhere in this file."""
import os

import numpy as np
import pytest
import torch
import yaml

from test_event_voxel_cpu import bits, golden_cases, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENSOR = (480, 640)


def synth_events(n, seed, H=480, W=640, ticks=100000):
    """n time-ordered synthetic events (numpy fp32 x, y, t, p) over and around an (H, W) sensor: fractional coordinates from -1.5 to
    half a pixel past the far edges, microsecond ticks with many equal timestamps, and a hot-pixel tail - 2 % of the events on 8
    pixels (a quarter of a percent, up to ten thousand events, on one cell)."""
    r = np.random.default_rng(seed)
    x, y = r.uniform(-1.5, W + 0.5, n), r.uniform(-1.5, H + 0.5, n)
    hot = r.permutation(n)[:n // 50]
    px, py = r.uniform(0, W - 1, 8), r.uniform(0, H - 1, 8)
    px[:4], py[:4] = np.floor(px[:4]), np.floor(py[:4])
    which = r.integers(0, 8, hot.size)
    x[hot], y[hot] = px[which], py[which]
    t = np.sort(r.integers(0, ticks, n)).astype(np.float32)
    t[0], t[-1] = 0, ticks
    return {"x": x.astype(np.float32), "y": y.astype(np.float32), "t": t, "p": r.integers(0, 2, n).astype(np.float32)}


def dev(ev):
    return {k: torch.from_numpy(v).to(DEV) for k, v in ev.items()}


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def test_fixture_bit_for_bit_both_modes():
    from sdformerflow_amd.DSEC_dataloader.event_representations import VoxelGrid
    for name, size, ev, chw, pol in golden_cases():
        got = VoxelGrid(size).convert_CHW(dev(ev))
        assert got.shape == chw.shape and np.array_equal(bits(got), bits(chw)), name
        got = VoxelGrid(size).convert_CHW_polarities(dev(ev))
        assert got.shape == pol.shape and np.array_equal(bits(got), bits(pol)), name


@pytest.mark.parametrize("n", [100000, 1000000, 4000000])
@pytest.mark.parametrize("C", [10, 20])
def test_full_size_equals_the_restatement_and_itself(C, n):
    """480 x 640: the grid equals the in-order restatement bit for bit; two runs are bit-equal; and a list gives the same bits whichever
    batch it is part of."""
    from sdformerflow_amd import hip
    ev = synth_events(n, seed=C * 7 + n % 1000 + 1)
    want = restate(ev["x"], ev["y"], ev["t"], ev["p"], (C,) + SENSOR)
    d = dev(ev)
    one = hip.event_voxel(d["x"], d["y"], d["t"], d["p"], C, SENSOR)
    assert one.shape == (1, C) + SENSOR and same_bits(one[0], want)
    again = hip.event_voxel(d["x"], d["y"], d["t"], d["p"], C, SENSOR)
    assert same_bits(again, one)
    m = n // 3                                                               # a second list: the first third, with its own time range
    short = hip.event_voxel(d["x"][:m], d["y"][:m], d["t"][:m], d["p"][:m], C, SENSOR)
    assert same_bits(short[0], restate(ev["x"][:m], ev["y"][:m], ev["t"][:m], ev["p"][:m], (C,) + SENSOR))
    cat = lambda k, order: torch.cat([d[k] if full else d[k][:m] for full in order])
    for order in ((True, False), (False, True), (False, True, False)):
        offs = np.concatenate(([0], np.cumsum([n if full else m for full in order]))).tolist()
        got = hip.event_voxel(cat("x", order), cat("y", order), cat("t", order), cat("p", order), C, SENSOR, offsets=offs)
        for i, full in enumerate(order):
            assert same_bits(got[i], one[0] if full else short[0]), (order, i)


def test_polarities_at_full_size():
    from sdformerflow_amd import hip
    ev = synth_events(1000000, seed=5)
    d = dev(ev)
    got = hip.event_voxel(d["x"], d["y"], d["t"], d["p"], 10, SENSOR, mode="polarities")
    assert same_bits(got[0], restate(ev["x"], ev["y"], ev["t"], ev["p"], (10,) + SENSOR, polarities=True))


@pytest.mark.parametrize("norm,spike_th", [("minmax", None), (None, None), ("minmax", 0.25), (None, 0.5), ("std", None)])
def test_model_input_equals_prepare_chunk_of_the_cropped_grid(norm, spike_th):
    """Output (b): crop, polarity split, normalisation, threshold fused - equal to harness.prepare_chunk(center_crop(grid)), one list
    and a batch of two (min-max runs over the whole batch tensor, as prepare_chunk's does)."""
    from sdformerflow_amd import harness, hip
    crop = (288, 384)
    a, b = dev(synth_events(1000000, seed=21)), dev(synth_events(300000, seed=22))
    for lists in ([a], [a, b]):
        grid = torch.cat([hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 10, SENSOR) for e in lists])
        want = harness.prepare_chunk(harness.center_crop(grid, crop), norm, spike_th)
        got = harness.events_to_chunk(lists if len(lists) > 1 else lists[0], 10, SENSOR, crop, norm, spike_th)
        assert got.shape == (len(lists), 10, 2) + crop and want.abs().sum() > 0
        assert same_bits(got, want), (norm, spike_th, len(lists))
        if norm is None and spike_th is None:                                # the cropped grid itself, computed on the window only
            cropped = hip.event_voxel(*(torch.cat([e[k] for e in lists]) for k in "xytp"), 10, SENSOR, crop=crop,
                                      offsets=np.concatenate(([0], np.cumsum([e["t"].numel() for e in lists]))).tolist())
            assert same_bits(cropped, harness.center_crop(grid, crop))


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint16])
def test_fused_rectification_equals_the_gather_in_torch(dtype):
    from sdformerflow_amd import hip
    from sdformerflow_amd.DSEC_dataloader.event_representations import rectify_events
    n, (H, W) = 500000, SENSOR
    ev = synth_events(n, seed=31)
    r = np.random.default_rng(32)
    xi, yi = r.integers(0, W, n), r.integers(0, H, n)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    rmap = np.stack((jj + r.uniform(-3, 3, (H, W)), ii + r.uniform(-3, 3, (H, W))), -1).astype(np.float32)   # some land outside
    rmap_d, t, p = torch.from_numpy(rmap).to(DEV), torch.from_numpy(ev["t"]).to(DEV), torch.from_numpy(ev["p"]).to(DEV)
    npt = np.int32 if dtype == torch.int32 else np.uint16
    xs, ys = (torch.from_numpy(v.astype(npt)).to(DEV) for v in (xi, yi))
    assert xs.dtype == dtype
    got = hip.event_voxel(xs, ys, t, p, 10, SENSOR, rectify_map=rmap_d)
    xr, yr = rectify_events(*(torch.from_numpy(v.astype(np.int64)).to(DEV) for v in (xi, yi)), rmap_d)
    assert same_bits(got, hip.event_voxel(xr, yr, t, p, 10, SENSOR))
    assert same_bits(got[0], restate(rmap[yi, xi, 0], rmap[yi, xi, 1], ev["t"], ev["p"], (10,) + SENSOR))


def test_no_events_and_degenerate_time():
    from sdformerflow_amd import harness, hip
    e = torch.empty(0, device=DEV)
    z = hip.event_voxel(e, e, e, e, 10, SENSOR)
    assert z.shape == (1, 10) + SENSOR and not z.any() and not bits(z).any()
    z = hip.event_voxel(e, e, e, e, 10, SENSOR, mode="polarities")
    assert z.shape == (1, 10, 2) + SENSOR and not z.any()
    got = harness.events_to_chunk({"x": e, "y": e, "t": e, "p": e}, 10, SENSOR, (288, 384), "minmax", 0.5)
    assert same_bits(got, harness.prepare_chunk(torch.zeros((1, 10, 288, 384), device=DEV), "minmax", 0.5))
    d = dev(synth_events(1000, seed=41))
    both = hip.event_voxel(d["x"], d["y"], d["t"], d["p"], 10, SENSOR, offsets=[0, 0, 1000, 1000])   # empty lists in a batch
    assert not both[0].any() and not both[2].any() and same_bits(both[1:2], hip.event_voxel(d["x"], d["y"], d["t"], d["p"], 10, SENSOR))
    flat = torch.full_like(d["t"], 7.0)                                      # t[N-1] == t[0]: the reference returns NaN; here an argument error
    with pytest.raises(hip.SdfError) as err:
        hip.event_voxel(d["x"], d["y"], flat, d["p"], 10, SENSOR)
    assert err.value.rc == hip.E_SHAPE
    with pytest.raises(hip.SdfError):                                        # ... also as the second list of a batch
        hip.event_voxel(torch.cat((d["x"], d["x"])), torch.cat((d["y"], d["y"])), torch.cat((d["t"], flat)), torch.cat((d["p"], d["p"])),
                        10, SENSOR, offsets=[0, 1000, 2000])


TINY = (8, 12)


def tiny_lists():
    """name -> one list on the 8 x 12 sensor at 2 bins: three events at half-pixel x, integer y and t_norm 0 | 0 | 1, so that every
    non-zero cell of the split is the one float 0.5 (min == max: nothing is normalised); and the empty list (no non-zero at all)."""
    three = {"x": [2.5, 6.5, 9.5], "y": [3.0, 5.0, 1.0], "t": [0.0, 0.0, 1.0], "p": [1.0, 0.0, 1.0]}
    return {"one value": {k: torch.tensor(v, dtype=torch.float32, device=DEV) for k, v in three.items()},
            "empty": {k: torch.empty(0, device=DEV) for k in "xytp"}}


@pytest.mark.parametrize("spike_th", [None, 0.25, 0.5])
@pytest.mark.parametrize("name", ["one value", "empty"])
def test_minmax_over_one_value_and_over_nothing(name, spike_th):
    """The min / max pair's two edge states - min == max, and no non-zero element - leave the split un-normalised, as
    harness.prepare_chunk of the signed grid does (0.5 against the thresholds: above 0.25 -> 1, equal to 0.5 -> kept)."""
    from sdformerflow_amd import harness, hip
    e = tiny_lists()[name]
    grid = hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 2, TINY)
    split = harness.prepare_chunk(grid, None, None)
    assert grid.shape == (1, 2) + TINY and set(split[split != 0].tolist()) == ({0.5} if name == "one value" else set())
    assert int((split != 0).sum()) == (6 if name == "one value" else 0) and (name == "empty" or (split[:, :, 1] != 0).any())
    got = hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 2, TINY, mode="split", norm="minmax", spike_th=spike_th)
    assert same_bits(got, harness.prepare_chunk(grid, "minmax", spike_th)), (name, spike_th)


def test_launch_log_names_the_kernels_of_a_call():
    from routes_common import logged
    from sdformerflow_amd import hip
    e = tiny_lists()["one value"]
    names = lambda rows: [r.split(" ", 3)[3].split("<")[0] for r in rows]
    rows, _ = logged(lambda: hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 2, TINY, mode="split", norm="minmax", check=False))
    assert names(rows) == ["ev_keys_kernel", "event_runs_kernel", "ev_gather_kernel", "ev_finish_kernel"], rows
    rows, _ = logged(lambda: hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 2, TINY, check=False))
    assert names(rows) == ["ev_keys_kernel", "event_runs_kernel", "ev_gather_kernel"], rows


def lif_model():
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4
    from sdformerflow_amd.synthetic import synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"]["input_size"] = [288, 384]
    model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    return model.to(DEV).eval(), cfg


def test_events_in_flow_out_equals_the_voxel_path():
    """events_to_chunk -> model gives the flow of the same model fed prepare_chunk(center_crop(grid)), bit for bit (lif, 288 x 384); so
    does forward_replicas on a batch of event lists; and evaluate on the event dict DSECDatasetLite yields equals evaluate on the grid."""
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.spikingjelly_compat import functional
    from sdformerflow_amd.synthetic import synth_label
    model, cfg = lif_model()
    crop = (288, 384)
    lists = [dev(synth_events(600000, seed=51)), dev(synth_events(400000, seed=52))]
    grids = [hip.event_voxel(e["x"], e["y"], e["t"], e["p"], 10, SENSOR) for e in lists]

    def flows(x, replicas=False):
        functional.reset_net(model)
        with torch.no_grad():
            return (model.forward_replicas(x) if replicas else model(x))["flow"]
    want = flows(harness.prepare_chunk(harness.center_crop(grids[0], crop)))
    got = flows(harness.events_to_chunk(lists[0], 10, SENSOR, crop, "minmax", None))
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)) and want[-1].abs().sum() > 0
    want = flows(harness.prepare_chunk(harness.center_crop(torch.cat(grids), crop)), replicas=True)
    got = flows(harness.events_to_chunk(lists, 10, SENSOR, crop, "minmax", None), replicas=True)
    assert all(same_bits(g, w) and g.shape[0] == 2 for g, w in zip(got, want))
    # evaluate: the raw dict of DSECDatasetLite (integer microsecond 'ts', normalised as the reference's preprocessing does)
    label, mask = synth_label(1, 480, 640)
    cfg["loader"]["crop"], cfg["metrics"] = list(crop), {"mask_events": True, "flow_scaling": 1}
    ev = lists[0]
    ts = ev["t"].to(torch.int64) + 1700000000
    sample = ({"ts": ts.cpu(), "x": ev["x"].cpu(), "y": ev["y"].cpu(), "p": ev["p"].cpu()}, mask[0], label[0])
    res = harness.evaluate(model, [sample], cfg, device=DEV)
    grid = hip.event_voxel(ev["x"], ev["y"], harness.event_times(ts), ev["p"], 10, SENSOR)
    assert res == harness.evaluate(model, [(grid.cpu(), mask, label)], cfg, device=DEV) and res["AEE"] > 0
