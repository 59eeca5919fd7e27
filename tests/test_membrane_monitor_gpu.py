"""The membrane monitor (sdformerflow_amd/monitor.py MembraneMonitor: the reference's `vis.monitor_v`) on the unfused HIP plan
(engine_unfused.py), MS_SpikingformerFlowNet with 3 encoders, lif, synthetic weights, keep="all", at 144 x 192, batch 1 and 2.

1. `names` and `elements` equal a FiringRateMonitor's on the same model and input; every call is recorded once.
2. For every call the table equals the numpy statistics (monitor.membrane_record) of the kept v_seq: exact.
3. The spikes of the SAME forward (the engine's tape runs beside the monitor) pass the spike-forced oracle replay (tests/replay.py)
   with 0 unexplained decisions.
4. For every call the kept v_seq agrees with the oracle's membrane at that call: the replay hook's pre-activation x, stepped on the CPU
   in fp32 with the forced spikes as the reset.  See V_TOL below.
5. The monitored flows against the plain fused forward's: finite, right shape; the difference is reported (profiles/).
6. One plif model and one hard-reset lif model through (1) and (2).
Then the harness entry, the CSV and the refusals (before any launch), and that a plain forward launches the same kernels before and
after a monitored one."""
import csv
import functools
import os

import numpy as np
import pytest
import torch
import yaml

import replay
from oracle import sdformer_oracle as O
from sdformerflow_amd import harness, hip
from sdformerflow_amd.monitor import FiringRateMonitor, MembraneMonitor, membrane_record
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet, SpikingformerFlowNet
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
SUFFIX = ".spiking_neuron"
V_TH = 0.1
# max |v_seq - oracle membrane| per neuron call.  Both sides step the SAME spikes (forced), so they differ by what the pre-activations
# differ by: the rounding of the products in front of the call (fp16 hi + lo weight planes, fp32 accumulation in another order), carried
# through at most T charge steps that each halve it (tau = 2) - no chaos, no threshold in between.  A wrong step axis, reset form or
# layout permutation moves a membrane by the order of v_th = 0.1, so the bound has to stay below 1e-2 * v_th = 1e-3 (the issue's
# condition).  Measured once on the MI355X over both inputs (profiles/membrane_vs_oracle.txt has the per-call maxima): 6.676e-6 at
# batch 1 and 6.676e-6 at batch 2, each at an `mlp.sn1` of the last stage (768 channels: the longest sums, membranes of order 1).
# V_TOL is 4 x that maximum rounded up to one digit, 4 x 6.676e-6 = 2.67e-5 -> 3e-5: 33 times below the cap.
V_TOL_CAP = 1e-2 * V_TH
V_TOL = 3e-5
EN3 = dict(swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])


def config(kind, size, v_reset=None, T=10):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=T, **({} if v_reset is None else {"v_reset": v_reset}))
    cfg["model"]["num_bins"] = 10
    cfg["swin_transformer"].update(input_size=list(size), window_size=[2, 9, 9])
    cfg["swin_transformer"].update(EN3)
    return cfg


@functools.lru_cache(maxsize=None)
def ms_model(kind, v_reset=None):
    """-> (model on the GPU, oracle state dict, oracle config), built as tests/test_firing_rate_gpu.py builds them."""
    cfg = config(kind, (144, 192), v_reset)
    model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(sd, strict=True)
    ocfg = {"neuron": O.NeuronCfg(kind, V_TH, v_reset, 2.0, 10), "num_bins": 10, "window_size": (2, 9, 9), "depths": EN3["swin_depths"],
            "num_heads": EN3["swin_num_heads"]}
    return model.eval().to(DEV), {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, ocfg


def stepped(x, s, ncfg):
    """The oracle's membrane at a call: its pre-activation x (T, ...) stepped in fp32 with the spikes s as the reset (soft reset)."""
    assert ncfg.neuron_type == "lif" and ncfg.v_reset is None
    v, out = torch.zeros_like(x[0]), []
    for t in range(x.shape[0]):
        h = v + (x[t] - v) / ncfg.tau
        v = h - s[t] * ncfg.v_th
        out.append(v)
    return torch.stack(out)


def table_check(mon):
    """(2): every call's records of the LAST forward equal the numpy statistics of its kept v_seq, integer for integer."""
    tab = mon.table()[-1].cpu().numpy()
    bad = []
    for i, name in enumerate(mon.names):
        v = mon.v_seq(name).cpu().numpy()                         # reference order: the steps first
        want = membrane_record(v, mon.lo, mon.hi, mon.bins)
        T = v.shape[0]
        if not (np.array_equal(tab[i, :T], want) and v[0].size == mon.elements[i]):
            bad.append((name, tab[i, :T, :4].tolist(), want[:, :4].tolist()))
        fresh = tab[i, T:]
        assert (fresh[:, 2] == 0xFFFFFFFF).all() and int(np.abs(np.delete(fresh, 2, axis=1)).sum()) == 0, name
    assert not bad, bad[:3]


@functools.lru_cache(maxsize=None)
def case(B):
    """One monitored + taped forward of the lif model on a batch of B, its oracle replay, a firing-rate monitor's forward and a plain
    forward: shared by the tests below."""
    model, sd, ocfg = ms_model("lif")
    chunk = harness.prepare_chunk(synth_voxel(B, 10, 144, 192, seed=77 + B))
    x = chunk.to(DEV)
    plain = model(x)["flow"]
    fr = FiringRateMonitor(model)
    with fr:
        model(x)
    mon = MembraneMonitor(model, keep="all")
    vref, kept = {}, {}

    def oracle_call():
        inner = O.NEURON_HOOK                                    # replay's forcing hook: sees every call first

        def hook(prefix, xx, s, ncfg, sd_):
            out = inner(prefix, xx, s, ncfg, sd_)
            name = prefix.rstrip(".")
            assert name not in vref, name
            vref[name] = stepped(xx, out, ncfg)
            if name.endswith(("attn.sn_k" + SUFFIX, "attn.sn2_q" + SUFFIX)):
                kept[name] = (out, ncfg)
            return out
        O.NEURON_HOOK = hook
        flows = O.forward_flownet(chunk, sd, ocfg, [])
        # the oracle runs `attn_sn` for the last block of a stage only: the others here, on the same gated tensor
        for name in [n for n in list(vref) if n.endswith("attn.sn_k" + SUFFIX)]:
            p = name[:-len("sn_k" + SUFFIX)]
            if p + "attn_sn" + SUFFIX in vref:
                continue
            k, (a, ncfg2) = kept[name][0], kept[p + "sn2_q" + SUFFIX]
            Tq, B_, N1, Cc = k.shape
            nH = a.shape[-1]
            e = k * a.repeat_interleave(Cc // nH, dim=-1)
            z = e.reshape(B_, nH, Tq, N1, Cc // nH).permute(2, 0, 3, 1, 4).reshape(Tq, B_, N1, Cc)
            O.attention_score(z, sd, p, ncfg2)
        return flows

    eng = model.unfused_engine()
    with mon:
        flows, ref, report = replay.run_part(eng, lambda: model(x)["flow"], oracle_call)
    return dict(model=model, mon=mon, fr=fr, flows=flows, plain=plain, vref=vref, summary=replay.summarise(report), B=B)


@pytest.mark.parametrize("B", [1, 2])
def test_names_and_elements_are_the_firing_rate_monitors(B):
    c = case(B)
    mon, fr = c["mon"], c["fr"]
    assert mon.names == fr.names and mon.elements == fr.elements and mon.forwards == 1 and not mon.enabled
    assert len(mon.names) == 6 + 10 * 7 + 2 + 4 + 6
    assert mon.table().shape == (1, len(mon.names), 10, 4 + 64 + 2) and mon.table().is_cuda


@pytest.mark.parametrize("B", [1, 2])
def test_table_equals_the_numpy_statistics_of_the_kept_v_seq(B):
    table_check(case(B)["mon"])


@pytest.mark.parametrize("B", [1, 2])
def test_spikes_of_the_monitored_forward_pass_the_oracle_replay(B):
    s = case(B)["summary"]
    print(s)
    assert s["unexplained"] == 0 and s["layers_forced"] >= 6 + 10 * 5 + 2 + 4 + 6, s


@pytest.mark.parametrize("B", [1, 2])
def test_v_seq_agrees_with_the_oracle_membrane(B):
    c = case(B)
    mon, vref = c["mon"], c["vref"]
    assert set(vref) == set(mon.names)
    dev = {}
    for name in mon.names:
        v, r = mon.v_seq(name).cpu(), vref[name]
        assert v.numel() == r.numel() and v.shape[0] == r.shape[0], (name, tuple(v.shape), tuple(r.shape))
        dev[name] = float((v.reshape(r.shape) - r).abs().max())
    for name in mon.names:
        print(f"batch {B} {name:95s} max|dv| {dev[name]:.3e}")
    worst = max(dev, key=dev.get)
    print(f"batch {B}: max |v_seq - oracle membrane| over {len(dev)} calls: {dev[worst]:.3e} at {worst}")
    assert V_TOL < V_TOL_CAP
    assert dev[worst] <= V_TOL, (worst, dev[worst])


@pytest.mark.parametrize("B", [1, 2])
def test_monitored_flows_against_the_plain_forward(B):
    c = case(B)
    diff = [float((a - b).abs().max()) for a, b in zip(c["flows"], c["plain"])]
    print(f"batch {B}: max |monitored flow - plain fused flow| per scale: {diff}; plain max |flow| {[float(p.abs().max()) for p in c['plain']]}")
    assert len(c["flows"]) == 3 and all(f.shape == (B, 2, 144, 192) and torch.isfinite(f).all() for f in c["flows"])


@pytest.mark.parametrize("kind,v_reset", [("plif", None), ("lif", 0.0)], ids=["plif", "lif_hard_reset"])
def test_plif_and_hard_reset_models(kind, v_reset):
    model, _, _ = ms_model(kind, v_reset)
    x = harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=81)).to(DEV)
    fr = FiringRateMonitor(model)
    with fr:
        model(x)
    mon = MembraneMonitor(model, keep="all")
    with mon:
        flows = model(x)["flow"]
    assert mon.names == fr.names and mon.elements == fr.elements
    assert all(torch.isfinite(f).all() for f in flows)
    table_check(mon)


def launches(fn):
    with hip.launch_log() as log:
        fn()
        torch.cuda.synchronize()
    return [(r[0], r[1], r[2]) for r in log.rows]


def test_harness_csv_refusals_and_the_untouched_plain_forward(tmp_path):
    model, _, _ = ms_model("lif")
    x = harness.prepare_chunk(synth_voxel(2, 10, 144, 192, seed=5)).to(DEV)
    before = launches(lambda: model(x[:1]))
    assert before and not any("vseq" in k or "membrane_stats" in k for k, _, _ in before)
    cfg = config("lif", (144, 192))
    cfg.setdefault("loader", {})["crop"] = None
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    label, mask = synth_label(1, 144, 192)
    samples = [(synth_voxel(1, 10, 144, 192, seed=5), mask, label), (synth_voxel(1, 10, 144, 192, seed=6), mask, label)]
    cfg["vis"] = {"monitor_v": False}
    off = harness.evaluate(model, samples, cfg, device=DEV)
    assert set(off) == {"AEE", "PE1", "PE2", "PE3", "outliers"}
    cfg["vis"] = {"monitor_v": True}
    mon = MembraneMonitor(model, bins=8)
    on = harness.evaluate(model, samples, cfg, device=DEV, monitor=mon)
    assert set(on) == set(off) | {"membrane"} and not mon.enabled and model._fr_monitor is None and mon.forwards == 2
    assert list(on["membrane"]) == mon.names
    first = on["membrane"][mon.names[0]]
    assert set(first) == {"mean", "min", "max", "hist", "n_nan"} and len(first["mean"]) == 10 and len(first["hist"][0]) == 8 + 2
    assert all(sum(h) == 2 * mon.elements[0] for h in first["hist"]) and all(lo <= m <= hi for lo, m, hi in zip(first["min"], first["mean"], first["max"]))
    assert len(on["membrane"][[n for n in mon.names if ".attn." in n][0]]["mean"]) == 2
    assert "membrane" in harness.evaluate(model, samples, cfg, device=DEV)                # a monitor of the loop's own
    # CSV round trip
    path = tmp_path / "membrane.csv"
    mon.to_csv(path)
    rows = list(csv.reader(open(path)))
    steps = sum(2 if ".attn." in n else 10 for n in mon.names)
    assert len(rows) == 2 * steps and rows[0][:4] == ["0", mon.names[0], "0", str(mon.elements[0])] and len(rows[0]) == 8 + 8 + 2
    tab = mon.table().cpu().numpy()
    assert float(rows[0][5]) == tab[0, 0, 0, 1] / 65536 / mon.elements[0] and [int(v) for v in rows[0][8:]] == tab[0, 0, 0, 4:].tolist()
    mon.reset()
    assert mon.forwards == 0 and mon.table().shape[0] == 0 and mon.summary() == {}

    # refusals: each before any launch
    def refused(exc, match, fn):
        with hip.launch_log() as log:
            with pytest.raises(exc, match=match):
                fn()
        assert log.rows == [], (match, log.rows[:3])
    both = dict(cfg, vis={"monitor_v": True, "monitor_fr": True})
    refused(RuntimeError, "monitor_fr and vis.monitor_v", lambda: harness.evaluate(model, samples, both, device=DEV))
    refused(RuntimeError, "monitor_v", lambda: harness.evaluate_stream(model, [], cfg, device=DEV))
    with mon:
        refused(RuntimeError, "forward_replicas", lambda: model.forward_replicas(x))
        refused(RuntimeError, "another MembraneMonitor", lambda: MembraneMonitor(model).enable())
        refused(RuntimeError, "another MembraneMonitor", lambda: FiringRateMonitor(model).enable())
        try:
            model.train()
            refused(RuntimeError, "training mode", lambda: model(x[:1]))
        finally:
            model.eval()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with pytest.raises((hip.SdfError, RuntimeError), match="graph capture"):
                with torch.cuda.graph(g, stream=s):
                    model(x[:1])
        torch.cuda.synchronize()
    assert mon.forwards == 0
    with FiringRateMonitor(model):
        refused(RuntimeError, "another FiringRateMonitor", lambda: mon.enable())
    for kind in ("psn", "glif"):
        other = MS_SpikingformerFlowNet(config(kind, (144, 192))["model"].copy(), config(kind, (144, 192))["swin_transformer"].copy())
        refused(hip.SdfError, "no membrane sequence", lambda: MembraneMonitor(other))
    sew = SpikingformerFlowNet.__new__(SpikingformerFlowNet)                              # (the class is enough: refused by type)
    refused(hip.SdfError, "SEW family", lambda: MembraneMonitor(sew))
    from sdformerflow_amd.STSwinNet.STSwinNet import STTFlowNet
    refused(hip.SdfError, "spiking model", lambda: MembraneMonitor(STTFlowNet.__new__(STTFlowNet)))
    long_model = MS_SpikingformerFlowNet.__new__(MS_SpikingformerFlowNet)
    torch.nn.Module.__init__(long_model)
    long_model.sttmultires_unet = type("U", (), {"spiking_kwargs": {"neuron_type": "lif", "v_th": 0.1}, "steps": 65, "window_size": (2, 9, 9),
                                                 "encoders": model.sttmultires_unet.encoders, "resblocks": [], "decoders": []})()
    refused(hip.SdfError, "at most 64", lambda: MembraneMonitor(long_model))
    # the plain forward of the same model launches what it launched before the monitored ones
    model(x[:1])                                                    # (train() above dropped the packed plan: this forward packs it again)
    assert launches(lambda: model(x[:1])) == before
