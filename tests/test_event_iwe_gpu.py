"""The image of warped events on the GPU (csrc/event_iwe.hip through hip.event_iwe / iwe_stats, loss.flow_warp, harness.warp_events and
the two loops' fwl=True) against the numpy restatement of tests/iwe_cases.py.  Every parity check is bit for bit - the same fp32
operations in the same order give the same bits - so there is no tolerance in them; the one bound of this file is hip.iwe_stats on a
bilinear image against numpy's fp64 sums (1e-12 relative: fp64 sums of at most 1280 fp32 values in another order)."""
import os

import numpy as np
import pytest
import torch

import iwe_cases as K
from routes_common import logged
from test_event_voxel_cpu import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                      # bytes of 0xA5 on either side of a guarded buffer (keeps its 256-byte alignment)


def dev(ev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in ev.items()}


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def guarded(nbytes):
    """(buffer, view of `nbytes` bytes between two guards, check)"""
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)

    def check():
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all()), "guard bytes were overwritten"
    return buf, buf[GUARD:GUARD + nbytes], check


def default_origin():
    (H, W), (h, w) = K.PARITY_SENSOR, K.PARITY_CROP
    return (H - h) // 2, (W - w) // 2


@pytest.fixture(scope="module")
def parity_case():
    """origin -> (the three lists: empty, one event, 20 000 events; their flows (3, 2, 32, 40)); computed once, left unchanged."""
    cases = {}
    for origin in ((3, 5), default_origin()):
        big = K.parity_events(origin)
        one = {k: v[7:8].copy() for k, v in big.items()}
        empty = {k: v[:0].copy() for k, v in big.items()}
        flows = np.stack([K.parity_flow(12), K.parity_flow(13), K.parity_flow(12)])
        cases[origin] = ([empty, one, big], flows)
    return cases


def batch(lists):
    cat = {k: np.concatenate([e[k] for e in lists]) for k in "xytp"}
    return dev(cat), np.concatenate(([0], np.cumsum([e["t"].size for e in lists]))).tolist()


def test_the_parity_case_holds_what_it_is_for(parity_case):
    lists, flows = parity_case[(3, 5)]
    big, flow = lists[2], flows[2]
    assert (np.diff(big["t"]) == 0).sum() > 1000 and (big["x"] < -1).any() and (big["x"] > K.PARITY_SENSOR[1]).any()
    assert not np.isfinite(flow).all() and np.isnan(flow).any() and np.isinf(flow).any()
    near = K.restate(big["x"], big["y"], big["t"], big["p"], flow, (3, 5), mode="nearest")
    (r0, c0, n0), (r1, c1, n1) = K.HOT
    assert near[0, r0, c0] >= n0 and near[0, r1, c1] >= n1 and n1 >= 48 and n0 > 128        # a long run and one of several chunks ...
    assert r0 == r1 and (r0 * K.PARITY_CROP[1] + c0) // 64 == (r1 * K.PARITY_CROP[1] + c1) // 64          # ... on lanes of one wave
    assert near.sum() < 0.9 * big["t"].size                                                  # events leave the window
    # exact integers and exact halves among the warped coordinates: integer pixels of the (2, 1) block at tau 0.25 | 0.5 | 0.75
    (b0, b1), (a0, a1) = K.FLOW_BLOCK
    block = np.isin(big["t"], (125, 250, 375)) & (big["x"] - 5 >= a0) & (big["x"] - 5 < a1) & (big["y"] - 3 >= b0) & (big["y"] - 3 < b1)
    assert block.sum() >= 100 and (big["x"][block] == np.rint(big["x"][block])).all()
    bil = K.restate(big["x"], big["y"], big["t"], big["p"], flow, (3, 5))
    assert bil.sum() > 0 and not np.array_equal(bil, near)


@pytest.mark.parametrize("t_ref,window", [(1.0, (0.0, 1.0)), (0.0, (0.0, 1.0)), (0.5, (0.5, 1.0))])
@pytest.mark.parametrize("origin", [(3, 5), None])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_parity_with_the_restatement(parity_case, mode, origin, t_ref, window):
    """Three lists in one call - empty, a single event (no time range: with check=False it adds nothing, in the restatement as well),
    20 000 events - equal the restatement bit for bit."""
    from sdformerflow_amd import hip
    at = origin or default_origin()
    lists, flows = parity_case[at]
    d, offs = batch(lists)
    got = hip.event_iwe(d["x"], d["y"], d["t"], d["p"], torch.from_numpy(flows).to(DEV), K.PARITY_SENSOR, offsets=offs,
                        crop=K.PARITY_CROP, crop_origin=origin, scale=1.0, t_ref=t_ref, window=window, mode=mode, check=False)
    torch.cuda.synchronize()
    assert got.shape == (3, 2) + K.PARITY_CROP
    for i, (ev, flow) in enumerate(zip(lists, flows)):
        want = K.restate(ev["x"], ev["y"], ev["t"], ev["p"], flow, at, 1.0, t_ref, window, mode)
        assert same_bits(got[i], want), (i, mode, origin, t_ref, window)
    assert not got[0].any() and not got[1].any() and got[2].sum() > 1000
    with pytest.raises(hip.SdfError) as err:                                 # the single-event list has no time range: refused when checked
        hip.event_iwe(d["x"], d["y"], d["t"], d["p"], torch.from_numpy(flows).to(DEV), K.PARITY_SENSOR, offsets=offs,
                      crop=K.PARITY_CROP, crop_origin=origin, mode=mode)
    assert err.value.rc == hip.E_SHAPE


def test_scale_multiplies_the_flow_and_the_whole_sensor_is_a_window(parity_case):
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    big = lists[2]
    d = dev(big)
    H, W = K.PARITY_SENSOR
    flow = np.zeros((2, H, W), dtype=np.float32)
    flow[:, 3:35, 5:45] = np.nan_to_num(flows[2], nan=0.0, posinf=9.0, neginf=-9.0)
    for mode in ("bilinear", "nearest"):
        got = hip.event_iwe(d["x"], d["y"], d["t"], d["p"], torch.from_numpy(flow[None]).to(DEV), (H, W), scale=0.37, mode=mode)
        assert same_bits(got[0], K.restate(big["x"], big["y"], big["t"], big["p"], flow, scale=0.37, mode=mode)), mode


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint16])
def test_integer_coordinates_through_a_rectify_map(parity_case, dtype):
    """x, y <- map[y, x] inside the kernel equals the gather done in torch, and the restatement on the gathered coordinates."""
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    big, flow = lists[2], flows[2]
    H, W = K.PARITY_SENSOR
    n = big["t"].size
    r = np.random.default_rng(32)
    xi, yi = r.integers(0, W, n), r.integers(0, H, n)
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    rmap = np.stack((jj + r.uniform(-3, 3, (H, W)), ii + r.uniform(-3, 3, (H, W))), -1).astype(np.float32)     # some land outside
    npt = np.int32 if dtype == torch.int32 else np.uint16
    xs, ys = (torch.from_numpy(v.astype(npt)).to(DEV) for v in (xi, yi))
    rmap_d, t, p, flow_d = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (rmap, big["t"], big["p"], flow[None]))
    xr, yr = rmap_d[ys.long(), xs.long(), 0].contiguous(), rmap_d[ys.long(), xs.long(), 1].contiguous()
    for mode in ("bilinear", "nearest"):
        got = hip.event_iwe(xs, ys, t, p, flow_d, (H, W), crop=K.PARITY_CROP, crop_origin=(3, 5), mode=mode, rectify_map=rmap_d)
        assert same_bits(got, hip.event_iwe(xr, yr, t, p, flow_d, (H, W), crop=K.PARITY_CROP, crop_origin=(3, 5), mode=mode))
        assert same_bits(got[0], K.restate(rmap[yi, xi, 0], rmap[yi, xi, 1], big["t"], big["p"], flow, (3, 5), mode=mode)) and got.sum() > 1000


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_runs_are_identical_and_a_list_does_not_depend_on_its_batch(parity_case, mode):
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    second = K.parity_events((3, 5), n=5000, seed=21)
    lists = [lists[2], lists[0], second]
    flows = np.stack([flows[2], flows[0], flows[1]])
    kw = dict(crop=K.PARITY_CROP, crop_origin=(3, 5), mode=mode, t_ref=0.5)
    d, offs = batch(lists)
    flows_d = torch.from_numpy(flows).to(DEV)
    both = hip.event_iwe(d["x"], d["y"], d["t"], d["p"], flows_d, K.PARITY_SENSOR, offsets=offs, **kw)
    again = hip.event_iwe(d["x"], d["y"], d["t"], d["p"], flows_d, K.PARITY_SENSOR, offsets=offs, **kw)
    assert torch.equal(both.view(torch.int32), again.view(torch.int32))
    for i, ev in enumerate(lists):
        e = dev(ev)
        alone = hip.event_iwe(e["x"], e["y"], e["t"], e["p"], flows_d[i:i + 1], K.PARITY_SENSOR, **kw)
        assert torch.equal(alone[0].view(torch.int32), both[i].view(torch.int32)), i
    assert both[0].sum() > 1000 and both[2].sum() > 1000 and not both[1].any()


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_out_and_workspace_keep_inside_their_buffers(parity_case, mode):
    """`out` and the workspace of exactly the size the library asks for lie between guard bytes, which stay as they were."""
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    d, offs = batch(lists)
    n, (H, W), (h, w) = d["t"].numel(), K.PARITY_SENSOR, K.PARITY_CROP
    need = hip.lib().sdf_event_iwe_workspace_bytes(n, 3, H, W, h, w, 3, 5, hip.EVENT_IWE_MODES[mode])
    assert need > 0
    ws_buf, ws, ws_check = guarded(need)
    out_buf, out_bytes, out_check = guarded(3 * 2 * h * w * 4)
    out = out_bytes.view(torch.float32).view(3, 2, h, w)
    key = (str(d["t"].device), torch.cuda.current_stream(d["t"].device).cuda_stream)
    kept = hip._IWE_WS.get(key)
    hip._IWE_WS[key] = ws
    try:
        got = hip.event_iwe(d["x"], d["y"], d["t"], d["p"], torch.from_numpy(flows).to(DEV), K.PARITY_SENSOR, offsets=offs,
                            crop=K.PARITY_CROP, crop_origin=(3, 5), mode=mode, check=False, out=out)
        torch.cuda.synchronize()
        assert hip._IWE_WS[key] is ws                                        # (the call used this buffer: it was large enough)
    finally:
        if kept is None:
            del hip._IWE_WS[key]
        else:
            hip._IWE_WS[key] = kept
    assert got is out
    ws_check()
    out_check()
    big = lists[2]
    assert same_bits(out[2], K.restate(big["x"], big["y"], big["t"], big["p"], flows[2], (3, 5), mode=mode))


def test_launch_log_names_the_new_kernels(parity_case):
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    d, offs = batch(lists)
    flows_d = torch.from_numpy(flows).to(DEV)
    call = lambda mode: hip.event_iwe(d["x"], d["y"], d["t"], d["p"], flows_d, K.PARITY_SENSOR, offsets=offs, crop=K.PARITY_CROP,
                                      crop_origin=(3, 5), mode=mode, check=False)
    rows, out = logged(lambda: call("bilinear"))
    # (a keys launch per non-empty list, then the run table with the permutation, then the gather)
    assert [r.split(" ", 3)[3].split("<")[0] for r in rows] == ["iwe_keys_kernel", "iwe_keys_kernel", "event_runs_kernel", "iwe_gather_kernel"], rows
    rows, near = logged(lambda: call("nearest"))
    assert [r.split(" ", 3)[3].split("<")[0] for r in rows] == ["iwe_keys_kernel", "iwe_keys_kernel", "event_runs_kernel", "iwe_gather_kernel"], rows
    rows, _ = logged(lambda: hip.iwe_stats(near))
    assert [r.split(" ", 3)[3].split("<")[0] for r in rows] == ["iwe_stats_partial_kernel", "iwe_stats_finish_kernel"], rows
    rows, _ = logged(lambda: hip.event_iwe(d["x"], d["y"], d["t"], d["p"], flows_d, K.PARITY_SENSOR, offsets=offs, crop=K.PARITY_CROP,
                                           crop_origin=(3, 5), window=(1.0, 0.0)))
    assert rows == [f"rc {hip.E_SHAPE}"]                                     # refused: nothing launched


def test_iwe_stats(parity_case):
    """Exactly the integer sums on nearest images; within 1e-12 relative of numpy's fp64 on a bilinear one; other rows untouched."""
    from sdformerflow_amd import hip
    lists, flows = parity_case[(3, 5)]
    d, offs = batch(lists)
    flows_d = torch.from_numpy(flows).to(DEV)
    images = {m: hip.event_iwe(d["x"], d["y"], d["t"], d["p"], flows_d, K.PARITY_SENSOR, offsets=offs, crop=K.PARITY_CROP,
                               crop_origin=(3, 5), mode=m, check=False) for m in ("nearest", "bilinear")}
    table = torch.full((6, 4), -7.0, dtype=torch.float64, device=DEV)
    assert hip.iwe_stats(images["nearest"], table=table, row=2) is table
    rows = table.cpu().numpy()
    assert (rows[:2] == -7).all() and (rows[5:] == -7).all()
    for i in range(3):
        img = images["nearest"][i].cpu().numpy()
        s1, s2 = K.int_stats(img)
        c = img.astype(np.float64).sum(0)
        assert rows[2 + i].tolist() == [float(s1), float(s2), float(c.max()), float((c != 0).sum())], i
    assert rows[4][0] > 1000 and rows[4][2] >= K.HOT[0][2]
    got = hip.iwe_stats(images["bilinear"]).cpu().numpy()
    alone = hip.iwe_stats(images["bilinear"][2:3]).cpu().numpy()
    assert np.array_equal(got[2], alone[0])                                  # a sample's record does not depend on its batch
    for i in range(3):
        c = images["bilinear"][i].cpu().numpy().astype(np.float64).sum(0)
        want = [c.sum(), (c * c).sum(), c.max(), float((c != 0).sum())]
        print("bilinear stats", i, got[i].tolist(), want)
        assert got[i][2] == want[2] and got[i][3] == want[3]
        assert abs(got[i][0] - want[0]) <= 1e-12 * abs(want[0]) and abs(got[i][1] - want[1]) <= 1e-12 * abs(want[1])
    # a larger image: many tiles per sample, a last tile that is not full
    big = torch.from_numpy(np.random.default_rng(3).integers(0, 5, (2, 2, 150, 201)).astype(np.float32)).to(DEV)
    got = hip.iwe_stats(big).cpu().numpy()
    for i in range(2):
        s1, s2 = K.int_stats(big[i].cpu().numpy())
        assert got[i][0] == s1 and got[i][1] == s2 and got[i][2] == big[i].sum(0).max().item()


def test_fwl_of_the_moving_dots_equals_the_restatement():
    from sdformerflow_amd import hip
    from sdformerflow_amd.loss.flow_warp import FWL, FlowWarpMetrics
    ev, flow = K.moving_dots()
    want = [K.fwl(ev["x"], ev["y"], ev["t"], ev["p"], f) for f in (flow, np.zeros_like(flow), -flow)]
    assert want[0] > 1.5 and want[1] == 1.0 and want[2] < 0.9
    d = dev(ev)
    flows = torch.from_numpy(np.stack([flow, np.zeros_like(flow), -flow])).to(DEV)
    got = FWL(flows, [d, d, d], K.DOTS_WINDOW, None, 1.0)()
    assert isinstance(got, tuple) and got[0].dtype == torch.float64 and got[0].tolist() == want
    # flow_scaling multiplies the prediction; a batch-1 call; the accumulator beside it
    assert FWL(flows[:1] / 4, d, K.DOTS_WINDOW, None, 4.0)()[0].tolist() == want[:1]
    acc = FlowWarpMetrics(2, DEV)
    rows, _ = logged(lambda: acc.update(flows[:1], d, K.DOTS_WINDOW, None, 1.0))
    assert any("iwe_stats" in r for r in rows)
    acc.update(flows[1:], [d, d], K.DOTS_WINDOW, None, 1.0)                 # (grows its tables)
    res = acc.result()
    assert res["FWL_samples"] == want and res["FWL"] == sum(want) / 3
    # half the window: other events, another value; an empty list has no variance
    half = FWL(flows[:1], d, K.DOTS_WINDOW, None, 1.0, window=(0.5, 1.0))()[0].item()
    assert half == K.fwl(ev["x"], ev["y"], ev["t"], ev["p"], flow, window=(0.5, 1.0)) and half != want[0]
    e = torch.empty(0, device=DEV)
    assert torch.isnan(FWL(flows[:1], {"x": e, "y": e, "t": e, "p": e}, K.DOTS_WINDOW, None, 1.0)()[0]).all()
    assert hip.E_SHAPE == -2


# -- the loops ---------------------------------------------------------------------------------------------------------------------
SENSOR, CROP = (150, 200), (144, 192)
FLOW_SCALING = 128


def loop_events(n, seed, mv=False):
    """n time-ordered events over the sensor as a loader yields them (host tensors): DSEC - integer microsecond 'ts', fp32 x / y;
    MV - float64 epoch seconds, integer pixels."""
    r = np.random.default_rng(seed)
    H, W = SENSOR
    x, y = r.integers(0, W, n), r.integers(0, H, n)
    ticks = np.sort(r.integers(0, 100000, n))
    ticks[0], ticks[-1] = 0, 100000
    p = torch.from_numpy(r.integers(0, 2, n).astype(np.float32))
    if mv:
        return {"ts": torch.from_numpy(1.5e9 + ticks * 1e-6), "x": torch.from_numpy(x.astype(np.int32)),
                "y": torch.from_numpy(y.astype(np.int32)), "p": p}
    return {"ts": torch.from_numpy(ticks + 1700000000), "x": torch.from_numpy(x.astype(np.float32)),
            "y": torch.from_numpy(y.astype(np.float32)), "p": p}


@pytest.fixture(scope="module")
def model_cfg():
    """The 3-encoder lif model at 144 x 192 with synthetic weights (tests/test_visualization_gpu.py's)."""
    import yaml
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
    from sdformerflow_amd.synthetic import synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"].update(input_size=list(CROP), swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    cfg["loader"] = dict(cfg["loader"], crop=list(CROP), polarity=True, resolution=list(SENSOR))
    cfg["data"] = dict(cfg["data"], num_chunks=2, num_frames=5)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": FLOW_SCALING, "name": ["AEE", "AAE"]}
    cfg["vis"] = dict(cfg.get("vis") or {}, store=False, enabled=False, monitor_fr=False, monitor_v=False)
    model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    return model.eval().to(DEV), cfg


def predictions(model, cfg, samples, mv):
    """The last flow level of every sample from a plain forward, as the loop forms its input."""
    from sdformerflow_amd import harness
    from sdformerflow_amd.spikingjelly_compat import functional
    preds = []
    for s in samples:
        to_dev = lambda ev: {k: v.to(DEV) for k, v in ev.items()}
        if mv:
            x = harness.event_pairs_to_chunk([(to_dev(s["events_old"]), to_dev(s["events_new"]))], 5, SENSOR, CROP,
                                             cfg["model"].get("norm_input"), cfg["data"].get("spike_th"))
        else:
            x = harness.events_to_chunk(to_dev(s[0]), cfg["model"]["num_bins"], SENSOR, CROP, cfg["model"].get("norm_input"),
                                        cfg["data"].get("spike_th"))
        functional.reset_net(model)
        with torch.no_grad():
            preds.append(model(x)["flow"][-1])
    return preds


@pytest.mark.parametrize("mv", [False, True])
def test_loops_with_fwl(model_cfg, tmp_path, mv):
    """fwl=True adds "FWL" - the mean of FWL(...)() on the predictions of a plain run - and changes nothing else; with vis.store the
    iwe PNGs hold event_counts_image of the bilinear image; fwl=False launches no iwe kernel and returns the plain dict."""
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.loss.flow_warp import FWL
    from sdformerflow_amd.synthetic import synth_label
    from sdformerflow_amd.utils.png import read_png
    model, cfg = model_cfg
    samples = []
    for i in range(2):
        label, mask = synth_label(1, *SENSOR, seed=4321 + i)
        if mv:
            samples.append({"events_old": loop_events(30000, 70 + i, True), "events_new": loop_events(40000 + 5000 * i, 80 + i, True),
                            "flow": label[0], "valid": mask[0, 0]})
        else:
            samples.append((loop_events(60000 + 5000 * i, 60 + i), mask[0, 0], label[0]))
    loop = harness.evaluate_mv if mv else harness.evaluate
    with hip.launch_log() as log:
        plain = loop(model, samples, cfg, device=DEV)
    assert not any("iwe" in r[0] for r in log.rows) and "FWL" not in plain
    with hip.launch_log() as log:
        assert loop(model, samples, cfg, device=DEV, fwl=False) == plain
    assert not any("iwe" in r[0] for r in log.rows)
    with hip.launch_log() as log:
        got = loop(model, samples, cfg, device=DEV, fwl=True)
    assert any("iwe_gather_kernel" in r[0] for r in log.rows) and any("iwe_stats" in r[0] for r in log.rows)
    assert {k: v for k, v in got.items() if k != "FWL"} == plain and list(got)[:len(plain)] == list(plain)
    preds = predictions(model, cfg, samples, mv)
    origin = harness.center_crop_origin(SENSOR, CROP) if mv else None
    events = [{k: v.to(DEV) for k, v in (s["events_new"] if mv else s[0]).items()} for s in samples]
    each = [FWL(p, e, SENSOR, CROP, FLOW_SCALING, crop_origin=origin)()[0].item() for p, e in zip(preds, events)]
    print("FWL per sample", each, "loop", got["FWL"])
    assert all(np.isfinite(v) and v > 0 for v in each) and got["FWL"] == sum(each) / 2
    # another window: other events, and the loop passes it on
    part = loop(model, samples, cfg, device=DEV, fwl=True, fwl_window=(0.25, 0.75))
    each = [FWL(p, e, SENSOR, CROP, FLOW_SCALING, window=(0.25, 0.75), crop_origin=origin)()[0].item() for p, e in zip(preds, events)]
    assert part["FWL"] == sum(each) / 2
    # stored: the tree gains iwe/, one file per sample, beside the unchanged others
    on = dict(cfg, vis=dict(cfg["vis"], store=True))
    stored = loop(model, samples, on, device=DEV, store_dir=str(tmp_path), sequence="seq_w", fwl=True)
    assert stored == got
    top = tmp_path / "results" / "eval_0" / "seq_w"
    assert sorted(os.listdir(top)) == ["events", "flow", "gtflow", "iwe"]
    assert sorted(os.listdir(top / "iwe")) == ["%09d.png" % i for i in range(2)]
    for i, (p, e) in enumerate(zip(preds, events)):
        iwe = harness.warp_events(e, p, SENSOR, CROP, FLOW_SCALING, crop_origin=origin)
        assert iwe.shape == (1, 2) + CROP and iwe.sum() > 1000
        assert np.array_equal(read_png(str(top / "iwe" / ("%09d.png" % i))), hip.event_counts_image(iwe)[0].cpu().numpy()), i
    # without fwl the stored tree has no iwe/
    loop(model, samples, on, device=DEV, store_dir=str(tmp_path), sequence="seq_plain")
    assert sorted(os.listdir(tmp_path / "results" / "eval_0" / "seq_plain")) == ["events", "flow", "gtflow"]
