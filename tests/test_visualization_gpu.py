"""The rendering kernels (csrc/flow_render.hip) against the numpy restatement of tests/vis_cases.py - which equals the reference's own
outputs byte for byte (tests/test_visualization_cpu.py) - and the harness paths that use them.

Bounds.  The submission encoding and the event sums share every operation with the restatement: bit-equal.  Flow and event IMAGES:
the only arithmetic not shared is atan2f (the device's against numpy's), and the quantile's interpolation (torch's against numpy's),
each a few ulps of fp32; that moves a value of at most 255 in front of its rounding by under 1e-3, so a byte may differ by ONE, and
does so with a probability of about that size: every byte within 1, and at most 1 % of a case's bytes differing at all."""
import os

import numpy as np
import pytest
import torch

import vis_cases as V

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def golden():
    return np.load(V.GOLDEN)


def guarded(shape, dtype):
    """(out, check): a contiguous `shape` tensor of u8 or u16 between GUARD bytes of 0xA5 on either side, and their check."""
    n = int(np.prod(shape)) * (2 if dtype == torch.uint16 else 1)
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)

    def check():
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all()), "guard bytes were overwritten"
    return buf[GUARD:GUARD + n].view(dtype).view(shape), check


def shifted(a, floats):
    """`a` on the device at a base `floats` floats behind an allocation's (16-byte aligned) start: contiguous, same values."""
    flat = torch.zeros(a.size + floats, dtype=torch.float32, device=DEV)
    flat[floats:] = torch.from_numpy(a).reshape(-1).to(DEV)
    t = flat[floats:].view(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 * floats) % 16
    return t


def check_image(got, want, what):
    worst, share = V.byte_report(got, want)
    print(f"{what}: largest byte difference {worst}, share of differing bytes {share:.2e}")
    assert worst <= 1 and share <= 0.01, (what, worst, share)
    return share


def flow_image(flow, mask=None, shift=0, mask_shift=0):
    from sdformerflow_amd import hip
    B, _, H, W = flow.shape
    out, check = guarded((B, H, W, 3), torch.uint8)
    with hip.launch_log() as log:
        got = hip.flow_image(shifted(flow, shift), None if mask is None else shifted(mask, mask_shift), out=out)
    torch.cuda.synchronize()
    assert got is out
    names = [r[0] for r in log.rows]
    assert len(names) == 2 and "flow_render_minmax_kernel" in names[0] and "flow_render_image_kernel" in names[1], names
    check()
    return out.cpu().numpy()


# -- flow image --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", V.FLOW_FIXTURES)
def test_flow_image_fixture(golden, name):
    got = flow_image(golden[f"flow/{name}"][None])
    check_image(got[0], golden[f"flow_img/{name}"], name)
    if name in ("const", "zero"):
        assert not got.any()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,H,W", V.RANDOM_SHAPES)
def test_flow_image_random(B, H, W, shift):
    """shift 1: the base one float behind a 16-byte boundary (3 head pixels; a tail where H W - 3 is no multiple of 4).  33 x 65 is
    odd, so fy cannot share fx's alignment: the element-wise path."""
    flow = V.random_flow(B, H, W, seed=100 + H)
    got = flow_image(flow, shift=shift)
    for b in range(B):
        check_image(got[b], V.flow_image_ref(flow[b]), f"({B}, {H}, {W}) shift {shift} sample {b}")


@pytest.mark.parametrize("mask_shift", [0, 2])
def test_flow_image_masked(mask_shift):
    """The mask is multiplied in first; mask_shift 2 puts it at another alignment than the flow (element-wise path)."""
    flow = V.random_flow(3, 16, 24, seed=7)
    mask = (np.random.default_rng(8).random((3, 1, 16, 24)) < 0.7).astype(np.float32)
    got = flow_image(flow, mask, mask_shift=mask_shift)
    for b in range(3):
        check_image(got[b], V.flow_image_ref(flow[b], mask[b, 0]), f"masked, mask shift {mask_shift}, sample {b}")
    assert not got[mask[:, 0] == 0].any()                       # (a masked pixel has magnitude 0, the sample's minimum: black)


def test_flow_image_samples_are_independent_and_runs_identical():
    """Sample b of a batch = the same sample rendered alone (the min / max words do not leak across samples), byte for byte, also
    where many workgroups share a sample's words; and a second call gives the same bytes."""
    from sdformerflow_amd import hip
    for B, H, W in ((3, 16, 24), (2, 33, 65), (2, 288, 384)):
        flow = torch.from_numpy(V.random_flow(B, H, W, seed=11 + H)).to(DEV)
        both = hip.flow_image(flow)
        again = hip.flow_image(flow)
        assert torch.equal(both, again)
        for b in range(B):
            assert torch.equal(hip.flow_image(flow[b:b + 1])[0], both[b]), (B, H, W, b)
        assert not torch.equal(both[0], both[1])


# -- submission --------------------------------------------------------------------------------------------------------------------
def submission(flow, shift=0):
    from sdformerflow_amd import hip
    B, _, H, W = flow.shape
    out, check = guarded((B, H, W, 3), torch.uint16)
    with hip.launch_log() as log:
        hip.flow_submission(shifted(flow, shift), out=out)
    torch.cuda.synchronize()
    assert len(log.rows) == 1 and "flow_render_submission_kernel" in log.rows[0][0], log.rows
    check()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", V.FLOW_FIXTURES)
def test_submission_fixture(golden, name):
    assert np.array_equal(submission(golden[f"flow/{name}"][None])[0], golden[f"sub/{name}"])


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,H,W", V.RANDOM_SHAPES)
def test_submission_random_is_bit_exact(B, H, W, shift):
    flow = V.random_flow(B, H, W, seed=200 + H)
    flow[0, :, 0, :4] = ((255.99, -255.99, 300.0, -300.0), (0.0, -0.0, 1e9, -1e9))          # the range's ends, and beyond them: clamped
    got = submission(flow, shift)
    for b in range(B):
        assert np.array_equal(got[b], V.submission_ref(flow[b])), (B, H, W, shift, b)
    assert got[0, 0, 2, 0] == 65535 and got[0, 0, 3, 0] == 0 and got[0, 0, 2, 1] == 65535 and got[0, 0, 3, 1] == 0


# -- event image -------------------------------------------------------------------------------------------------------------------
def event_image(src, window=None):
    """(bytes, counts) of hip.event_image / event_counts on `src` (numpy), the output between guard bytes."""
    from sdformerflow_amd import hip
    t = torch.from_numpy(src).to(DEV)
    h, w = window[2:] if window else src.shape[-2:]
    out, check = guarded((src.shape[0], h, w, 3), torch.uint8)
    kw = dict(crop=(h, w), crop_origin=window[:2]) if window else {}
    with hip.launch_log() as log:
        hip.event_image(t, out=out, **kw)
    torch.cuda.synchronize()
    names = [r[0] for r in log.rows]
    assert len(names) == 2 and "flow_render_event_sum_kernel" in names[0] and "flow_render_event_image_kernel" in names[1], names
    check()
    return out.cpu().numpy(), hip.event_counts(t, **kw).cpu().numpy()


@pytest.mark.parametrize("name", V.EVENT_FIXTURES)
def test_event_image_fixture(golden, name):
    """The fixture's counts as a one-bin split input: the sums are the counts, the image the reference's float image rounded."""
    counts = golden[f"events/{name}"]
    got, summed = event_image(counts[None, None])
    assert np.array_equal(summed[0], counts)
    check_image(got[0], V.event_bytes_of(golden[f"events_img/{name}"]), name)


@pytest.mark.parametrize("B,bins,Hs,Ws,window", [(1, 10, 5, 7, None), (3, 10, 16, 24, None), (2, 20, 40, 70, (3, 5, 33, 65)),
                                                 (2, 10, 21, 33, (1, 3, 16, 24))])
def test_event_image_signed(B, bins, Hs, Ws, window):
    src = V.random_voxel(B, bins, Hs, Ws, seed=300 + Hs)
    got, summed = event_image(src, window)
    for b in range(B):
        counts = V.event_counts_ref(src[b], window)
        assert np.array_equal(summed[b], counts), b             # the same adds in the same order: bit-equal
        check_image(got[b], V.event_image_ref(counts), f"signed ({B}, {bins}, {Hs}, {Ws}) window {window} sample {b}")


@pytest.mark.parametrize("B,bins,Hs,Ws,window", [(2, 10, 33, 65, None), (1, 20, 21, 33, (1, 3, 16, 24))])
def test_event_image_split(B, bins, Hs, Ws, window):
    v = V.random_voxel(B, bins, Hs, Ws, seed=400 + Hs)
    src = np.stack([np.maximum(v, 0), np.maximum(-v, 0)], 2)
    got, summed = event_image(src, window)
    for b in range(B):
        counts = V.event_counts_ref(src[b], window)
        assert np.array_equal(summed[b], counts), b
        check_image(got[b], V.event_image_ref(counts), f"split ({B}, {bins}, {Hs}, {Ws}) window {window} sample {b}")


def test_event_image_samples_are_independent_and_runs_identical():
    from sdformerflow_amd import hip
    src = torch.from_numpy(V.random_voxel(3, 10, 33, 65, seed=9)).to(DEV)
    both = hip.event_image(src)
    assert torch.equal(both, hip.event_image(src))
    for b in range(3):
        assert torch.equal(hip.event_image(src[b:b + 1])[0], both[b]), b
    assert not torch.equal(both[0], both[1])


def test_python_surface_refusals():
    from sdformerflow_amd import hip
    flow = torch.zeros(2, 2, 4, 6, device=DEV)
    with hip.launch_log() as log:
        for call in (lambda: hip.flow_image(flow[:, :1]), lambda: hip.flow_image(flow, mask=torch.zeros(2, 1, 4, 5, device=DEV)),
                     lambda: hip.flow_image(flow, out=torch.zeros(2, 4, 6, 3, device=DEV)),
                     lambda: hip.flow_submission(flow, out=torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=DEV)),
                     lambda: hip.flow_image(flow.double()), lambda: hip.event_image(torch.zeros(1, 10, 3, 4, 6, device=DEV)),
                     lambda: hip.event_image(torch.zeros(1, 10, 4, 6, device=DEV), crop=(5, 6))):
            with pytest.raises(hip.SdfError):
                call()
    assert log.rows == []


# -- harness -----------------------------------------------------------------------------------------------------------------------
SENSOR, CROP = (150, 200), (144, 192)


@pytest.fixture(scope="module")
def model_cfg():
    """The 3-encoder MS model at 144 x 192 of tests/test_evaluate_stream_gpu.py, and 3 loader items at the sensor's size."""
    import yaml
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
    from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"].update(input_size=list(CROP), swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    cfg["loader"] = dict(cfg["loader"], crop=list(CROP), polarity=True)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    cfg["vis"] = dict(cfg.get("vis") or {}, store=False, enabled=False, monitor_fr=False, monitor_v=False)
    model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    samples = []
    for i in range(3):
        label, mask = synth_label(1, *SENSOR, seed=4321 + i)
        samples.append((synth_voxel(1, 10, *SENSOR, seed=40 + 3 * i), mask[:, 0], label))
    return model.eval().to(DEV), cfg, samples


def test_evaluate_stores_the_tree_and_changes_no_metric(model_cfg, tmp_path):
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.utils.png import read_png
    model, cfg, samples = model_cfg
    with hip.launch_log() as log:
        plain = harness.evaluate(model, samples, cfg, device=DEV, store_dir=str(tmp_path))
    assert not any("flow_render" in r[0] for r in log.rows) and not os.listdir(tmp_path)     # vis.store false: nothing rendered
    on = dict(cfg, vis=dict(cfg["vis"], store=True))
    stored = harness.evaluate(model, samples, on, device=DEV, store_dir=str(tmp_path), sequence="seq_a", submission=True)
    assert stored == plain
    top = tmp_path / "results" / "eval_0"
    assert sorted(os.listdir(top)) == ["flow_test", "seq_a"] and sorted(os.listdir(top / "seq_a")) == ["events", "flow", "gtflow"]
    for sub in ("events", "flow", "gtflow"):
        assert sorted(os.listdir(top / "seq_a" / sub)) == ["%09d.png" % i for i in range(3)]
    assert sorted(os.listdir(top / "flow_test" / "seq_a")) == ["%06d.png" % i for i in range(3)]
    for i, (vox, _, label) in enumerate(samples):
        v = harness.center_crop(vox.to(DEV), CROP)
        with torch.no_grad():
            pred = model(harness.prepare_chunk(v, cfg["model"].get("norm_input"), cfg["data"].get("spike_th"), True))["flow"][-1]
        lab = harness.center_crop(label.to(DEV), CROP).contiguous()
        name = "%09d.png" % i
        assert np.array_equal(read_png(str(top / "seq_a" / "flow" / name)), hip.flow_image(pred)[0].cpu().numpy())
        assert np.array_equal(read_png(str(top / "seq_a" / "gtflow" / name)), hip.flow_image(lab)[0].cpu().numpy())
        assert np.array_equal(read_png(str(top / "seq_a" / "events" / name)), hip.event_image(v)[0].cpu().numpy())
        sub = read_png(str(top / "flow_test" / "seq_a" / ("%06d.png" % i)))
        assert sub.dtype == np.uint16 and np.array_equal(sub, hip.flow_submission(pred)[0].cpu().numpy())
        assert np.array_equal(sub, V.submission_ref(pred[0].cpu().numpy()))


def test_evaluate_stream_fills_the_render_buffers(model_cfg):
    from sdformerflow_amd import harness, hip
    model, cfg, samples = model_cfg
    n, (h, w) = len(samples), CROP
    ev = harness.StreamEvaluator(model, cfg, DEV, replicas=2, streams=2)
    flows0 = torch.zeros((n, 2, h, w), device=DEV)
    res0 = ev.run(samples, flows_out=flows0)
    counts0 = ev.metrics.counts().clone()
    renders = {k: torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device=DEV) for k in ("flow", "gtflow", "events")}
    renders["submission"] = torch.full((n, h, w, 6), 0xA5, dtype=torch.uint8, device=DEV).view(torch.uint16)
    flows = torch.zeros_like(flows0)
    res = ev.run(samples, flows_out=flows, renders_out=renders)
    assert res == res0 and torch.equal(flows, flows0)
    assert torch.equal(ev.metrics.counts().view(torch.int64), counts0.view(torch.int64))
    assert torch.equal(renders["flow"], torch.cat([hip.flow_image(flows[i:i + 1]) for i in range(n)]))
    assert torch.equal(renders["submission"].view(torch.int16), hip.flow_submission(flows).view(torch.int16))
    for i, (vox, _, label) in enumerate(samples):
        lab = harness.center_crop(label.to(DEV), CROP).contiguous()
        assert torch.equal(renders["gtflow"][i], hip.flow_image(lab)[0]), i
        assert torch.equal(renders["events"][i], hip.event_image(vox.to(DEV), crop=CROP)[0]), i
    assert all(not torch.equal(renders[k][i].view(torch.uint8), renders[k][0].view(torch.uint8)) for k in renders for i in (1, 2))
    with pytest.raises(ValueError, match="unknown keys"):
        ev.run(samples, renders_out={"iwe": renders["flow"]})
    with pytest.raises(RuntimeError, match="renders_out"):
        harness.evaluate_stream(model, samples, dict(cfg, vis=dict(cfg["vis"], store=True)), device=DEV)
