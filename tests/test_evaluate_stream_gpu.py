"""harness.evaluate_stream: the benchmark's scheme (R batch-1 forwards per launch sequence, a HIP graph per stream, F streams) as a
library call, with input preparation and metrics on the device.  Geometry: the 3-encoder MS model at 144 x 192, the smallest
tests/test_replica_batch.py runs replicas on; 7 samples with replicas = 3 on 2 streams: a full graph on both streams and a remainder
graph of one sample."""
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu
SENSOR, CROP = (150, 200), (144, 192)


def build(kind, H, W):
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
    from sdformerflow_amd.synthetic import synth_state_dict
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"].update(input_size=[H, W], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    cfg["loader"] = dict(cfg["loader"], crop=[H, W], polarity=True)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    return model.eval().to(DEV), cfg


def tuples(n, size, seed0=40):
    """n loader items (voxel (1, 10, Hs, Ws), mask (1, Hs, Ws), label (1, 2, Hs, Ws)) on the host, every one its own."""
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    out = []
    for i in range(n):
        label, mask = synth_label(1, *size, seed=4321 + i)
        out.append((synth_voxel(1, 10, *size, seed=seed0 + 3 * i), mask[:, 0], label))
    return out


@pytest.fixture(scope="module")
def run():
    """One streamed evaluation of 7 samples, shared by the tests below and left unchanged."""
    from sdformerflow_amd import harness
    model, cfg = build("lif", *CROP)
    samples = tuples(7, SENSOR)
    flows = torch.full((7, 2) + CROP, float("nan"), device=DEV)
    ev = harness.StreamEvaluator(model, cfg, DEV, replicas=3, streams=2)
    res = ev.run(samples, flows_out=flows)
    return {"model": model, "cfg": cfg, "samples": samples, "flows": flows, "res": res, "counts": ev.metrics.counts().clone(), "ev": ev}


def test_flows_are_the_plain_forwards_bit_for_bit(run):
    from sdformerflow_amd import harness
    assert harness.stream_plan(7, 2, 3) == [(0, 0, 3), (1, 3, 3), (0, 6, 1)]
    assert sorted(run["ev"].slots[0]["fwd"]) == [1, 3] and sorted(run["ev"].slots[1]["fwd"]) == [3]       # the graphs that were used
    for k, (vox, _, _) in enumerate(run["samples"]):
        x = harness.prepare_chunk(harness.center_crop(vox.to(DEV), CROP), "minmax", None, True)
        with torch.no_grad():
            want = run["model"](x)["flow"][-1]
        assert torch.equal(run["flows"][k], want[0]), k
    assert not torch.equal(run["flows"][0], run["flows"][1])


def test_counts_are_the_kernel_on_those_flows(run):
    from sdformerflow_amd import harness, hip
    assert run["counts"].shape == (7, 8)
    for k, (_, mask, label) in enumerate(run["samples"]):
        lab, msk = harness.center_crop(label, CROP).to(DEV), harness.center_crop(mask, CROP).to(DEV)
        one = hip.flow_metrics(run["flows"][k:k + 1], lab, msk, None, 1)
        assert torch.equal(one.view(torch.int64), run["counts"][k:k + 1].view(torch.int64)), k


def check_against(res, ref):
    """PE1-3 / outliers: identical integer counts, divided in fp32 by evaluate and in fp64 here: 2^-23.  AEE: 1e-6 relative, the bound
    tests/test_harness.py uses between two fp32 summation orders.  AAE (evaluate_mv): the class sums N = 27 648 fp32 terms in a tree,
    ~ log2(N) 2^-24 = 9e-7 relative, and takes an acos of ~ 2 ulps per term: 1e-5 relative."""
    assert set(res) == set(ref)
    for key in ("PE1", "PE2", "PE3", "outliers"):
        assert abs(res[key] - ref[key]) <= 2.0 ** -23, (key, res[key], ref[key])
    assert abs(res["AEE"] - ref["AEE"]) <= 1e-6 * abs(ref["AEE"]), (res["AEE"], ref["AEE"])
    if "AAE" in ref:
        assert abs(res["AAE"] - ref["AAE"]) <= 1e-5 * abs(ref["AAE"]), (res["AAE"], ref["AAE"])


def test_result_is_evaluates(run):
    from sdformerflow_amd import harness
    ref = harness.evaluate(run["model"], run["samples"], run["cfg"], device=DEV)
    print("evaluate_stream", run["res"], "evaluate", ref)
    check_against(run["res"], ref)
    assert 0 < run["res"]["PE3"] < 1 and run["res"]["AEE"] > 0


def test_eager_issue_gives_the_same_table(run):
    from sdformerflow_amd import harness
    ev = harness.StreamEvaluator(run["model"], run["cfg"], DEV, replicas=3, streams=2, graphs=False)
    flows = torch.empty_like(run["flows"])
    res = ev.run(iter(run["samples"]), flows_out=flows)                    # (an iterator: no length known in advance)
    assert torch.equal(ev.metrics.counts().view(torch.int64), run["counts"].view(torch.int64)) and torch.equal(flows, run["flows"])
    assert res == run["res"] and ev.slots[0]["fwd"] == {}
    # the one-call form; other group sizes and stream counts number the samples the same way
    res2 = harness.evaluate_stream(run["model"], run["samples"], run["cfg"], device=DEV, replicas=2, streams=3, flows_out=flows)
    assert res2 == run["res"] and torch.equal(flows, run["flows"])


def test_mv_dict_form_with_event_mask_and_aae(run):
    """The MVSEC / MDR loader's volumes (old | new, 5 bins each), metrics.mask_events and AEE + AAE, against evaluate_mv."""
    from sdformerflow_amd import harness
    from sdformerflow_amd.synthetic import synth_label, synth_voxel
    cfg = dict(run["cfg"], data=dict(run["cfg"]["data"], num_chunks=2, num_frames=5),
               metrics={"mask_events": True, "flow_scaling": 1, "name": ["AEE", "AAE"]})
    items = []
    for i in range(4):
        label, mask = synth_label(1, *CROP, seed=77 + i)
        vol = synth_voxel(1, 10, *CROP, seed=900 + i, density=0.03)
        items.append({"event_volume_old": vol[:, :5], "event_volume_new": vol[:, 5:], "flow": label, "valid": mask[:, 0]})
    ev = harness.StreamEvaluator(run["model"], cfg, DEV, replicas=3, streams=2)
    res = ev.run(items)
    ref = harness.evaluate_mv(run["model"], items, cfg, device=DEV)
    print("evaluate_stream", res, "evaluate_mv", ref)
    check_against(res, ref)
    # the event mask took pixels away: fewer valid pixels than the labels' own masks have
    n_valid = ev.metrics.counts()[:, 0].cpu().numpy()
    own = np.array([float(it["valid"].sum()) for it in items])
    assert (n_valid < own).all() and (n_valid > 0).all()


def test_a_geometry_the_replica_tables_refuse_goes_one_by_one():
    """160 x 224 has an odd window count per sample at some stage: forward_replicas meets ReplicaGeometryError inside and serves the
    samples one by one - inside the captured graph as well.  Same numbers as evaluate."""
    from sdformerflow_amd import harness, hip
    model, cfg = build("lif", 160, 224)
    eng = model.engine()
    with pytest.raises(hip.ReplicaGeometryError), torch.no_grad():
        eng.forward(torch.zeros((2, 10, 2, 160, 224), device=DEV), None, replicas=True)
    samples = tuples(4, (160, 224), seed0=70)
    res = harness.evaluate_stream(model, samples, cfg, device=DEV, replicas=3, streams=2)
    check_against(res, harness.evaluate(model, samples, cfg, device=DEV))
