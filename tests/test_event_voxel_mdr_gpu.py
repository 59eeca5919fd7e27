"""The MVSEC / MDR event front end on the GPU (csrc/event_voxel_tb.hip through hip.event_voxel_tb, MDR_dataloader.loader_utils,
harness.event_pairs_to_chunk, harness.evaluate_mv) against the reference's own outputs (tests/golden/events_voxel_mdr.npz, written by
tests/golden/make_golden_events_mdr.py from the real class on the CPU).  Un-normalised grids are compared bit for bit; normalised ones
under a bound measured on the fixture (test_normalised_volumes_match_the_reference_within_its_own_error)."""
import os

import numpy as np
import pytest
import torch
import yaml

from test_event_voxel_mdr_cpu import bits, golden, golden_lists, measured_norm_error, normalise64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NB, SENSOR = 5, (36, 44)


def cols(events, dev=DEV):
    """(N, 4) float64 [ts, x, y, p] -> the raw event dict on the device."""
    ev = torch.from_numpy(np.ascontiguousarray(events)).to(dev)
    return {"ts": ev[:, 0].contiguous(), "x": ev[:, 1].to(torch.int32), "y": ev[:, 2].to(torch.int32), "p": ev[:, 3].to(torch.float32)}


def voxel(events, size, **kw):
    from sdformerflow_amd import hip
    c = cols(events)
    return hip.event_voxel_tb(c["x"], c["y"], c["ts"], c["p"], size[0], size[1:], t_scale=1e6, **kw)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def lists():
    return {name: (size, ev, ref) for name, size, ev, ref in golden_lists()}


@pytest.fixture(scope="module")
def bound():
    return 4.0 * measured_norm_error()


def pairs_of(lists):
    """Four (old, new) pairs out of the 5 x 36 x 44 lists: the stored pair, and the short, empty and single-event lists in both places."""
    return [(lists[o][1], lists[n][1]) for o, n in (("a", "b"), ("c", "e"), ("d", "a"), ("b", "c"))]


def test_unnormalised_volumes_are_the_reference_bits_and_reproducible(lists):
    for name, (size, ev, ref) in lists.items():
        one = voxel(ev, size, normalize=False)
        assert one.shape == (1,) + size and same_bits(one[0], ref["raw"]), name
        assert same_bits(voxel(ev, size, normalize=False), one), name
        pol = voxel(ev, size, normalize=False, mode="polarities")
        assert pol.shape == (1, size[0], 2) + size[1:] and same_bits(pol[0], ref["pol"]), name
        assert same_bits(voxel(ev, size, normalize=False, mode="polarities"), pol), name


def test_coordinate_dtypes_agree(lists):
    from sdformerflow_amd import hip
    size, ev, ref = lists["a"]
    c = cols(ev)
    for x, y in ((c["x"].float(), c["y"].float()), (c["x"].to(torch.uint16), c["y"].to(torch.uint16))):
        assert same_bits(hip.event_voxel_tb(x, y, c["ts"], c["p"], NB, SENSOR, t_scale=1e6, normalize=False)[0], ref["raw"])


def test_fp32_times_do_not_reproduce_the_fixture(lists):
    """The fixture detects an fp32 time path: epoch stamps rounded to fp32 collapse onto one value, and the grid is another one."""
    size, ev, ref = lists["a"]
    ev32 = ev.copy()
    ev32[:, 0] = ev[:, 0].astype(np.float32)
    assert not same_bits(voxel(ev32, size, normalize=False)[0], ref["raw"])
    assert same_bits(voxel(ev, size, normalize=False)[0], ref["raw"])


def test_out_of_range_events_add_nothing(lists):
    size, ev, ref = lists["a"]
    nb, H, W = size
    r = np.random.default_rng(5)
    at = np.sort(r.choice(len(ev) - 2, 40, replace=False)) + 1                  # (the first and the last event keep their places)
    extra = ev[at].copy()
    extra[:10, 1], extra[10:20, 1], extra[20:30, 2], extra[30:, 2] = W, -3, H, -1
    extra[5:8, 1], extra[25:28, 2] = 1 << 20, -(1 << 20)
    more = np.insert(ev, at, extra, axis=0)
    assert len(more) == len(ev) + 40 and (np.diff(more[:, 0]) >= 0).all()
    assert same_bits(voxel(more, size, normalize=False)[0], ref["raw"])
    assert same_bits(voxel(more, size, normalize=False, mode="polarities")[0], ref["pol"])


def test_normalised_volumes_match_the_reference_within_its_own_error(lists, bound):
    """The reference normalises in fp32 with torch's reductions; this package evaluates the same formula in float64 and rounds once.
    The bound is measured, not chosen: the largest absolute difference, over the fixture's lists, between the reference's normalised
    volumes and a float64 evaluation of its formula on its own un-normalised bits is 6.5e-7 (at values up to 19.8;
    measured_norm_error() recomputes it), and the bound is 4 x that = 2.6e-6.  The margin covers torch.std's reduction order, which is
    not part of the contract.  The pol=False form has its own measurement, 2.5e-6 at values up to 32.2, hence 1.0e-5.  Zero cells
    match exactly."""
    print("measured reference error %.3e, bound %.3e; pol=False form %.3e" % (bound / 4, bound, measured_norm_error("polarities")))
    assert 6.4e-7 < bound / 4 < 6.6e-7 and 2.5e-6 < measured_norm_error("polarities") < 2.6e-6       # (the figures quoted above)
    for name, (size, ev, ref) in lists.items():
        for mode, key, raw in (("signed", "norm", "raw"), ("polarities", "poln", "pol")):
            bound = 4.0 * measured_norm_error(mode)
            got = voxel(ev, size, normalize=True, mode=mode)[0].cpu().numpy()
            dev = float(np.abs(got.astype(np.float64) - ref[key]).max())
            exact = float(np.abs(got.astype(np.float64) - normalise64(ref[raw])).max())
            print(name, mode, "vs reference %.3e, vs float64 formula %.3e" % (dev, exact))
            assert dev <= bound, (name, mode, dev)
            assert np.array_equal(got == 0, ref[key] == 0), (name, mode)
            assert same_bits(voxel(ev, size, normalize=True, mode=mode)[0], got), (name, mode)


def test_crop_equals_the_slice_of_the_uncropped_result(lists):
    for name in ("a", "f"):
        size, ev, ref = lists[name]
        h, w = size[1] - 7, size[2] - 9
        for normalize in (False, True):
            for mode in ("signed", "polarities"):
                full = voxel(ev, size, normalize=normalize, mode=mode)
                part = voxel(ev, size, normalize=normalize, mode=mode, crop=(h, w), crop_origin=(2, 3))
                assert same_bits(part, full[..., 2:2 + h, 3:3 + w]), (name, normalize, mode)


def test_model_input_and_event_mask(lists, bound):
    """The fused model input against the reference loop's output under the measured bound (scaled: min-max divides by hi - lo, which
    is far above 1 here, so the absolute bound holds as it is), and bit for bit against prepare_chunk on the kernel's own volumes."""
    from sdformerflow_amd import harness
    z = golden()
    (size, old, _), (_, new, _) = lists["a"], lists["b"]
    pair = (cols(old), cols(new))
    chunk, mask = harness.event_pairs_to_chunk(pair, NB, SENSOR, None, "minmax", None, want_event_mask=True)
    assert chunk.shape == (1, 2 * NB, 2) + SENSOR and mask.shape == (1, 1) + SENSOR and mask.dtype == torch.float32
    dev = float((chunk.cpu() - torch.from_numpy(z["ab_chunk"])).abs().max())
    print("model input vs the reference loop: %.3e (bound %.3e)" % (dev, bound))
    assert dev <= bound
    assert np.array_equal(mask.cpu().numpy() != 0, z["ab_event_mask"])
    vols = torch.cat((voxel(old, size), voxel(new, size)), dim=1)                          # the kernel's own signed volumes
    for norm_input, th in (("minmax", None), ("minmax", 0.25), (None, None), (None, 0.5), ("std", None), ("std", 0.1)):
        got, m = harness.event_pairs_to_chunk(pair, NB, SENSOR, None, norm_input, th, want_event_mask=True)
        want = harness.prepare_chunk(vols, norm_input, th, True)
        assert same_bits(got, want), (norm_input, th)
        assert torch.equal(m != 0, want.sum(1).sum(1, keepdim=True).bool()), (norm_input, th)
        assert same_bits(harness.event_pairs_to_chunk(pair, NB, SENSOR, None, norm_input, th), want)
    one = harness.event_pairs_to_chunk(pair, NB, SENSOR, None, "minmax", None, num_chunks=1)
    assert same_bits(one, harness.prepare_chunk(voxel(new, size), "minmax", None, True))


TINY = (8, 12)


def tiny_pair(name):
    """(x, y, t, p, offsets) of an (old, new) pair on the 8 x 12 sensor at 2 bins.  "one value": three events on three pixels at
    t_norm 0 | 0 | 1 and an empty new list - every non-zero cell of the split is the one float 1 (min == max: nothing is normalised);
    "empty": two empty lists (no non-zero at all)."""
    n = 3 if name == "one value" else 0
    x, y = torch.tensor([2, 6, 9][:n], dtype=torch.int32, device=DEV), torch.tensor([3, 5, 1][:n], dtype=torch.int32, device=DEV)
    t = torch.tensor([0.0, 0.0, 1.0][:n], dtype=torch.float64, device=DEV)
    return x, y, t, torch.tensor([1.0, 0.0, 1.0][:n], dtype=torch.float32, device=DEV), [0, n, n]


@pytest.mark.parametrize("spike_th", [None, 1.0, 2.0])
@pytest.mark.parametrize("name", ["one value", "empty"])
def test_minmax_over_one_value_and_over_nothing(name, spike_th):
    """The min / max pair's two edge states - min == max, and no non-zero element - leave the split un-normalised, as
    harness.prepare_chunk of the signed volumes does (1 against the thresholds: equal to 1 -> kept, below 2 -> 0), and the event mask
    is chunk.sum(1).sum(1).bool()."""
    from sdformerflow_amd import harness, hip
    x, y, t, p, offs = tiny_pair(name)
    vols = hip.event_voxel_tb(x, y, t, p, 2, TINY, offsets=offs, normalize=False)
    vols = vols.reshape(1, 4, *TINY)                                                       # old | new along the bins
    split = harness.prepare_chunk(vols, None, None)
    assert set(split[split != 0].tolist()) == ({1.0} if name == "one value" else set())
    assert int((split != 0).sum()) == (3 if name == "one value" else 0) and (name == "empty" or (split[:, :, 1] != 0).any())
    got, mask = hip.event_voxel_tb(x, y, t, p, 2, TINY, offsets=offs, normalize=False, mode="split", lists_per_sample=2, norm="minmax",
                                   spike_th=spike_th, want_event_mask=True)
    want = harness.prepare_chunk(vols, "minmax", spike_th)
    assert got.shape == (1, 4, 2) + TINY and same_bits(got, want), (name, spike_th)
    assert mask.shape == (1, 1) + TINY and torch.equal(mask != 0, want.sum(1).sum(1, keepdim=True).bool()), (name, spike_th)
    assert bool(mask.any()) == (name == "one value" and spike_th != 2.0)


def test_launch_log_names_the_kernels_of_a_call():
    from routes_common import logged
    from sdformerflow_amd import hip
    x, y, t, p, offs = tiny_pair("one value")
    names = lambda rows: [r.split(" ", 3)[3].split("<")[0] for r in rows]
    rows, _ = logged(lambda: hip.event_voxel_tb(x, y, t, p, 2, TINY, offsets=offs, normalize=False, mode="split", lists_per_sample=2,
                                                norm="minmax", want_event_mask=True))
    # (a keys launch per non-empty list, the run table with the permutation, the gather, the split with min / max, the shared finish)
    assert names(rows) == ["tb_keys_kernel", "event_runs_kernel", "tb_gather_kernel", "tb_norm_kernel", "prepare_finish_kernel"], rows
    rows, _ = logged(lambda: hip.event_voxel_tb(x, y, t, p, 2, TINY, offsets=offs))
    # (signed volumes, normalised per list: the lists' statistics between the gather and the normalisation)
    assert names(rows) == ["tb_keys_kernel", "event_runs_kernel", "tb_gather_kernel", "tb_stats_kernel", "tb_norm_kernel"], rows


def test_batching_does_not_change_a_sample(lists):
    """Pairs one by one and as one batch of 4 give the same bits per sample before the batch-wide min-max; with it, the batch equals
    prepare_chunk on the concatenated per-sample outputs.  The crop (default centre origin) and the event mask ride along."""
    from sdformerflow_amd import harness
    pairs = [(cols(o), cols(n)) for o, n in pairs_of(lists)]
    crop = (32, 40)
    singles = [harness.event_pairs_to_chunk(p, NB, SENSOR, crop, None, None) for p in pairs]
    batch = harness.event_pairs_to_chunk(pairs, NB, SENSOR, crop, None, None)
    assert batch.shape == (4, 2 * NB, 2) + crop and same_bits(batch, torch.cat(singles))
    assert same_bits(harness.event_pairs_to_chunk(pairs, NB, SENSOR, crop, None, None), batch)
    full = harness.event_pairs_to_chunk(pairs, NB, SENSOR, None, None, None)
    assert harness.center_crop_origin(SENSOR, crop) == (2, 2) and harness.center_crop_origin((260, 346), (256, 256)) == (2, 45)
    assert same_bits(batch, full[..., 2:34, 2:42])
    got, mask = harness.event_pairs_to_chunk(pairs, NB, SENSOR, crop, "minmax", 0.3, want_event_mask=True)
    want = harness.prepare_chunk(torch.cat(singles), "minmax", 0.3, polarity=False)
    assert same_bits(got, want) and torch.equal(mask != 0, want.sum(1).sum(1, keepdim=True).bool())
    assert not got[2, :NB].any() and got[2, NB:].any()                                     # (the empty old list of the third pair)


def test_reference_call_form_returns_the_same_tensors(lists):
    import importlib
    import sdformerflow_amd
    from sdformerflow_amd import hip
    sdformerflow_amd.install_reference_aliases()
    lu = importlib.import_module("MDR_dataloader.loader_utils")
    for name in ("a", "c", "e"):
        size, ev, ref = lists[name]
        feats = torch.from_numpy(ev).to(DEV)
        keep = feats.clone()
        seq = lu.EventSequence(None, {"height": size[1], "width": size[2]}, features=feats, timestamp_multiplier=1e6, convert_to_relative=True)
        assert torch.equal(feats, keep) and len(seq) == len(ev) and float(seq.get_sequence_only()[0, 0]) == 0.0
        for kw, mode, key in ((dict(normalize=False), "signed", "raw"), (dict(normalize=False, pol=False), "polarities", "pol")):
            got = lu.EventSequenceToVoxelGrid_Pytorch(size[0], gpu=True, forkserver=False, **kw)(seq)
            assert same_bits(got, ref[key]), (name, mode)
        got = lu.EventSequenceToVoxelGrid_Pytorch(num_bins=size[0], normalize=True, gpu=True, pol=True)(seq)
        assert got.shape == size and same_bits(got, voxel(ev, size, normalize=True)[0]), name
    size, ev, ref = lists["a"]
    shuffled = torch.from_numpy(ev[np.random.default_rng(3).permutation(len(ev))]).to(DEV)      # unsorted: sorted by time, stably
    seq = lu.EventSequence(None, {"height": 36, "width": 44}, features=shuffled, timestamp_multiplier=1e6, convert_to_relative=True)
    assert seq.is_sorted()
    c = cols(ev, "cpu")
    with pytest.raises(hip.SdfError):
        hip.event_voxel_tb(c["x"], c["y"], c["ts"], c["p"], NB, SENSOR)
    with pytest.raises(hip.SdfError):
        hip.event_voxel_tb(*(cols(ev)[k] for k in ("x", "y", "ts", "p")), NB, SENSOR, crop=(32, 40), crop_origin=(5, 2))


def synth_pair(seed, n, size):
    """Two raw event lists (seconds, epoch) on a sensor of `size`."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(2):
        t = 1.5e9 + k * 0.05 + np.sort(r.integers(0, 40000, n)) * 1e-6
        out.append(np.stack([t, r.integers(0, size[1], n), r.integers(0, size[0], n), r.integers(0, 2, n)], axis=1).astype(np.float64))
    return out


def test_evaluate_mv_on_volumes_and_on_raw_events():
    """evaluate_mv with the smallest model tests/test_harness.py builds (the four-encoder SNN at 288 x 384, 2 x 5 bins): the same
    metrics whether a sample carries the loader's volumes or the raw event lists; mask_events changes the result only through the
    pixels whose event mask is zero."""
    import sdformerflow_amd
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4
    from sdformerflow_amd.loss.flow_supervised import AEE
    from sdformerflow_amd.synthetic import synth_label, synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"]["input_size"] = [288, 384]
    size, crop = (292, 390), (288, 384)
    cfg["loader"] = dict(cfg.get("loader", {}), crop=list(crop), resolution=list(size), polarity=True)
    cfg["data"] = dict(cfg["data"], num_chunks=2, num_frames=5)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1, "name": ["AEE", "AAE"]}
    model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model = model.to(DEV).eval()
    label, valid = synth_label(1, *crop)
    raw, vols = [], []
    oy, ox = harness.center_crop_origin(size, crop)
    for seed in (41, 42):
        old, new = synth_pair(seed, 20000, size)
        raw.append({"events_old": cols(old), "events_new": cols(new), "flow": label[0], "valid": valid[0]})
        v = [voxel(e, (5,) + size)[:, :, oy:oy + crop[0], ox:ox + crop[1]] for e in (old, new)]
        vols.append({"event_volume_old": v[0].cpu(), "event_volume_new": v[1].cpu(), "flow": label, "valid": valid})
    res_raw = harness.evaluate_mv(model, raw, cfg, device=DEV)
    res_vol = harness.evaluate_mv(model, vols, cfg, device=DEV)
    print("evaluate_mv raw", res_raw, "volumes", res_vol)
    assert set(res_raw) == {"AEE", "PE1", "PE2", "PE3", "outliers", "AAE"} and res_raw == pytest.approx(res_vol, rel=1e-6, abs=1e-9)
    assert all(np.isfinite(v) for v in res_raw.values()) and res_raw["AEE"] > 0
    cfg["metrics"]["mask_events"] = True
    masked_raw = harness.evaluate_mv(model, raw, cfg, device=DEV)
    assert masked_raw == pytest.approx(harness.evaluate_mv(model, vols, cfg, device=DEV), rel=1e-6, abs=1e-9)
    # what mask_events does, stated directly: the metric with valid * event mask, where the mask comes from the model's input
    tot = 0.0
    for s in raw:
        x, em = harness.event_pairs_to_chunk((s["events_old"], s["events_new"]), 5, size, crop, cfg["model"].get("norm_input"),
                                             cfg["data"].get("spike_th"), want_event_mask=True)
        assert 0 < float(em.sum()) < em.numel()
        sdformerflow_amd.spikingjelly_compat.functional.reset_net(model)
        with torch.no_grad():
            pred = model(x)["flow"][-1]
        tot += float(AEE(pred, label.to(DEV), valid.to(DEV).unsqueeze(1).float() * em, 1)()[0][0])
    assert abs(masked_raw["AEE"] - tot / 2) <= 1e-6 * abs(tot / 2) and masked_raw["AEE"] != res_raw["AEE"]
    with pytest.raises(hip.SdfError):
        harness.evaluate_mv(model, [dict(raw[0], events_old=cols(synth_pair(1, 10, size)[0], "cpu"), events_new=cols(synth_pair(1, 10, size)[1], "cpu"))],
                            cfg, device="cpu")
