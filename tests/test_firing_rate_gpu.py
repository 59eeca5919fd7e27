"""The firing-rate monitor (sdformerflow_amd/monitor.py: the reference's `vis.monitor_fr`) on the HIP forward.

1. Exact: the monitored forward's counts and denominators equal, integer for integer, the per-step spike sums `s.flatten(1).sum(1)`
   and `s[0].numel()` of every neuron call of the spike-forced oracle replay (tests/replay.py) of the same input - the forced GPU
   spikes in the reference's layout, the oracle's own for the calls the tape does not hold (the MS token gates and `attn_sn`).
2. The monitored forward's flows are the plain forward's, bit for bit.
3. The rates of the reference's own forward (fixtures end_to_end.npz / sew_end_to_end.npz: 105 / 75 calls) are met in call order.
4. harness.evaluate's two entries, the CSV.  5. The refusals."""
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
from sdformerflow_amd.monitor import FiringRateMonitor
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet, MS_SpikingformerFlowNet_en4, SpikingformerFlowNet
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
SUFFIX = ".spiking_neuron"
# |rate - fixture rate| per neuron call of a free-running forward: the chaotic net decorrelates after one flipped spike, the rates are
# statistics of it.  The project's bound for this fixture on a foreign host is 2e-3 (tests/test_oracle_golden.py).  Measured once on
# the MI355X over the four fixture forwards (profiles/firing_rate_vs_fixture.txt): maxima 1.708e-3 (en4 lif), 1.775e-3 (en4 psn),
# 2.379e-3 (SEW lif), 2.263e-3 (SEW psn), each at a small late-stage call; above 1e-3, so the bound is twice the measured maximum
# rounded up to one digit, 2 x 2.379e-3 -> 5e-3 (under the 1e-2 cap: a wrong denominator or step axis moves rates of 0.1 - 0.5 by more).
# That the COUNTS are right is the exact tests' business; this one pins names, order and denominators against the reference's own run.
RATE_TOL = 5e-3


def config(kind, size, T=10):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=T)
    cfg["model"]["num_bins"] = 10
    cfg["swin_transformer"].update(input_size=list(size), window_size=[2, 9, 9])
    return cfg


EN3 = dict(swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])


@functools.lru_cache(maxsize=None)
def ms_model(kind, size, en4):
    """-> (model on the GPU, oracle state dict, oracle config), built as tests/test_replay_gpu.py builds them."""
    cfg = config(kind, size)
    if not en4:
        cfg["swin_transformer"].update(EN3)
    cls = MS_SpikingformerFlowNet_en4 if en4 else MS_SpikingformerFlowNet
    model = cls(cfg["model"].copy(), cfg["swin_transformer"].copy())
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict(sd, strict=True)
    ocfg = {"neuron": O.NeuronCfg(kind, 0.1, None, 2.0, 10), "num_bins": 10, "window_size": (2, 9, 9),
            "depths": cfg["swin_transformer"]["swin_depths"], "num_heads": cfg["swin_transformer"]["swin_num_heads"]}
    return model.eval().to(DEV), {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}, ocfg


@functools.lru_cache(maxsize=None)
def sew_model(kind):
    cfg = config(kind, (144, 192))
    cfg["swin_transformer"].update(EN3)
    model = SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    sd = synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(("relative_position_index",))})
    model.load_state_dict(sd, strict=False)
    model = model.eval().to(DEV)
    sd = {k: v.cpu() for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    ocfg = {"neuron": O.NeuronCfg(kind, 0.1, None, 2.0, 10), "num_bins": 10, "window_size": (2, 9, 9), "depths": [2, 2, 6],
            "num_heads": [3, 6, 12]}
    return model, sd, ocfg


def replayed_calls(model, chunk, oracle_forward, sd, ms):
    """Spike-forced oracle replay of `chunk` with every neuron call's spikes summed per step in the reference's layout:
    -> (taped GPU flows, {call name: ((T,) int64 sums, elements per step)}).  MS family: the oracle runs `attn_sn` for the last block
    of a stage only; for the others it is run here on the same gated tensor, from the spikes the hook saw (forced k, the oracle's gate)."""
    seen, kept = {}, {}

    def oracle_call():
        inner = O.NEURON_HOOK                              # replay's forcing hook: sees every call first

        def hook(prefix, x, s, ncfg, sd_):
            out = inner(prefix, x, s, ncfg, sd_)
            name = prefix.rstrip(".")
            assert name not in seen, name
            seen[name] = (out.flatten(1).sum(1).to(torch.int64), out[0].numel())
            if name.endswith(("attn.sn_k" + SUFFIX, "attn.sn2_q" + SUFFIX)):
                kept[name] = (out, ncfg)
            return out
        O.NEURON_HOOK = hook
        flows = oracle_forward(chunk)
        if ms:
            for name in [n for n in list(seen) if n.endswith("attn.sn_k" + SUFFIX)]:
                p = name[:-len("sn_k" + SUFFIX)]
                if p + "attn_sn" + SUFFIX in seen:
                    continue
                k, (a, ncfg2) = kept[name][0], kept[p + "sn2_q" + SUFFIX]
                Tq, B_, N1, Cc = k.shape
                nH = a.shape[-1]
                e = k * a.repeat_interleave(Cc // nH, dim=-1)                                   # oracle qk_attention: the gate
                z = e.reshape(B_, nH, Tq, N1, Cc // nH).permute(2, 0, 3, 1, 4).reshape(Tq, B_, N1, Cc)
                O.attention_score(z, sd, p, ncfg2)
        return flows

    eng = model.engine()
    flows, ref, report = replay.run_part(eng, lambda: eng.forward(chunk.to(DEV)), oracle_call)
    assert replay.summarise(report)["unexplained"] == 0
    return flows, seen


def check_exact(model, sd, ocfg, chunk, oracle_forward, ms=True):
    x = chunk.to(DEV)
    mon = FiringRateMonitor(model)
    with mon:
        monitored = model(x)["flow"]
    assert mon.forwards == 1 and not mon.enabled
    flows, seen = replayed_calls(model, chunk, oracle_forward, sd, ms)
    plain = model(x)["flow"]
    # 2. the same forward: monitored == plain == taped, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(monitored, plain)), "the monitored forward differs from the plain one"
    assert all(torch.equal(a, b) for a, b in zip(monitored, flows))
    # 1. every call the oracle made and no other, counts and denominators exact
    assert set(mon.names) == set(seen) and len(mon.names) == len(seen)
    counts = mon.counts()
    assert counts.shape == (1, len(mon.names), mon.Tmax) and counts.dtype == torch.int64 and counts.is_cuda
    counts = counts[0].cpu()
    bad, recs = [], mon.records[0]
    for i, name in enumerate(mon.names):
        sums, n = seen[name]
        T = sums.numel()
        if not (torch.equal(counts[i, :T], sums) and int(counts[i, T:].abs().sum()) == 0 and mon.elements[i] == n):
            bad.append((name, counts[i].tolist(), sums.tolist(), mon.elements[i], n))
        assert recs[i].dtype == torch.float32 and torch.equal(recs[i], (sums.double() / n).float()), name
    assert not bad, bad[:4]
    gates = [i for i, n in enumerate(mon.names) if "sn2_q" in n]
    return mon, [float(counts[i].sum()) / (mon.elements[i] * 2) for i in gates]


def test_counts_equal_the_replayed_oracle_batch_of_two_lif():
    model, sd, ocfg = ms_model("lif", (144, 192), False)
    chunk = harness.prepare_chunk(synth_voxel(2, 10, 144, 192, seed=77))
    mon, gates = check_exact(model, sd, ocfg, chunk, lambda c: O.forward_flownet(c, sd, ocfg, []))
    assert len(mon.names) == 6 + 10 * 7 + 2 + 4 + 6 and len(gates) == 10
    print("lif token-gate rates:", ["%.3f" % g for g in gates])


def test_counts_equal_the_replayed_oracle_batch_of_two_psn():
    """The PSN model's token gates fire at intermediate rates: the recomputed gate is exercised non-trivially (the LIF gates sit at 1)."""
    model, sd, ocfg = ms_model("psn", (144, 192), False)
    chunk = harness.prepare_chunk(synth_voxel(2, 10, 144, 192, seed=78))
    mon, gates = check_exact(model, sd, ocfg, chunk, lambda c: O.forward_flownet(c, sd, ocfg, []))
    print("psn token-gate rates:", ["%.3f" % g for g in gates])
    assert any(0.05 < g < 0.95 for g in gates), gates


def test_counts_equal_the_replayed_oracle_odd_sizes():
    """150 x 200: padded windows at every stage, a zero row in front of every patch merging, cropped decoders - the denominators are
    the reference tensors' own, padding included."""
    model, sd, ocfg = ms_model("lif", (150, 200), False)
    chunk = harness.prepare_chunk(synth_voxel(1, 10, 150, 200, seed=93))
    check_exact(model, sd, ocfg, chunk, lambda c: O.forward_flownet(c, sd, ocfg, []))


def test_counts_equal_the_replayed_oracle_sew():
    model, sd, ocfg = sew_model("lif")
    chunk = harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=1234 + 7))
    mon, _ = check_exact(model, sd, ocfg, chunk, lambda c: O.forward_sew_flownet(c, sd, ocfg), ms=False)
    assert len(mon.names) == 75


def fixture_check(model, chunk, fixture, kind):
    g = np.load(os.path.join(HERE, "golden", fixture))
    mon = FiringRateMonitor(model)
    with mon:
        model(chunk.to(DEV))
        torch.cuda.synchronize()
    names, ref = [str(n) for n in g[f"{kind}_rate_names"]], g[f"{kind}_rates"].astype(np.float64)
    assert mon.names == names
    got = np.array([float(r.double().mean()) for r in mon.records[0]])
    dev = np.abs(got - ref)
    for n, a, b, d in zip(names, got, ref, dev):
        print(f"{fixture} {kind} {n:95s} gpu {a:.6f} fixture {b:.6f} dev {d:.2e}")
    mean_dev = abs(mon.mean() - float(ref.mean()))
    print(f"{fixture} {kind} max dev {dev.max():.3e} at {names[int(dev.argmax())]}; mean of rates: gpu {mon.mean():.6f} "
          f"fixture {ref.mean():.6f} dev {mean_dev:.2e}")
    assert dev.max() <= RATE_TOL, (names[int(dev.argmax())], float(dev.max()))
    assert mean_dev <= RATE_TOL
    return mon


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_rates_of_the_shipped_model_meet_the_reference_fixture(kind):
    """en4 at 288 x 384, the fixture's input: all 105 calls in the reference's order."""
    model, _, _ = ms_model(kind, (288, 384), True)
    mon = fixture_check(model, harness.prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1235)), "end_to_end.npz", kind)
    assert len(mon.names) == 105


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_rates_of_the_sew_model_meet_the_reference_fixture(kind):
    model, _, _ = sew_model(kind)
    mon = fixture_check(model, harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=1234 + 7)), "sew_end_to_end.npz", kind)
    assert len(mon.names) == 75


def test_harness_entries_and_csv(tmp_path):
    model, _, _ = ms_model("lif", (144, 192), False)
    cfg = config("lif", (144, 192))
    cfg.setdefault("loader", {})["crop"] = None
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    label, mask = synth_label(1, 144, 192)
    samples = [(synth_voxel(1, 10, 144, 192, seed=5), mask, label), (synth_voxel(1, 10, 144, 192, seed=6), mask, label)]
    cfg["vis"] = dict(cfg.get("vis") or {}, monitor_fr=False)
    off = harness.evaluate(model, samples, cfg, device=DEV)
    assert set(off) == {"AEE", "PE1", "PE2", "PE3", "outliers"}
    del cfg["vis"]
    assert harness.evaluate(model, samples, cfg, device=DEV) == off
    cfg["vis"] = {"monitor_fr": True}
    mon = FiringRateMonitor(model)
    assert mon.counts().shape == (0, len(mon.names), 10) and mon.counts().is_cuda            # empty, and where the model lies
    other = FiringRateMonitor(ms_model("psn", (144, 192), False)[0])
    with pytest.raises(ValueError, match="another model"):
        harness.evaluate(model, samples, cfg, device=DEV, monitor=other)
    assert not other.enabled and model._fr_monitor is None
    on = harness.evaluate(model, samples, cfg, device=DEV, monitor=mon)
    assert set(on) == set(off) | {"firing_rate", "firing_rates"} and all(on[k] == off[k] for k in off)
    assert not mon.enabled and model._fr_monitor is None and mon.forwards == 2
    assert on["firing_rate"] == mon.mean() and 0.0 < on["firing_rate"] < 1.0
    assert list(on["firing_rates"]) == mon.names
    recs = mon.records
    for i, name in enumerate(mon.names):
        want = (recs[0][i].double() + recs[1][i].double()) / 2
        assert np.allclose(on["firing_rates"][name], want.numpy(), rtol=0, atol=1e-7), name
        assert len(on["firing_rates"][name]) == (2 if ".attn." in name else 10)
    own = harness.evaluate(model, samples, cfg, device=DEV)                     # a monitor of the loop's own
    assert own["firing_rate"] == on["firing_rate"] and model._fr_monitor is None
    path = tmp_path / "firing_rate.csv"
    mon.to_csv(path)
    rows = list(csv.reader(open(path)))
    assert len(rows) == 2 * len(mon.names)
    assert rows[0][:2] == ["0", mon.names[0]] and rows[-1][:2] == ["1", mon.names[-1]] and len(rows[0]) == 2 + 10
    assert np.allclose([float(v) for v in rows[0][2:]], recs[0][0].numpy(), atol=1e-7)
    mon.to_csv(path)
    assert len(list(csv.reader(open(path)))) == 4 * len(mon.names)
    mon.reset()
    assert mon.forwards == 0 and mon.records == [] and mon.counts().shape[0] == 0


def test_table_grows_without_losing_records():
    model, _, _ = ms_model("lif", (144, 192), False)
    x = harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=5)).to(DEV)
    mon = FiringRateMonitor(model, forwards=1)
    with mon:
        for _ in range(3):
            model(x)
    c = mon.counts()
    assert c.shape[0] == 3 and torch.equal(c[0], c[1]) and torch.equal(c[0], c[2]) and int(c[0].sum()) > 0
    model.invalidate_engine()                                                   # the monitor lives on the model: a rebuilt engine keeps it
    with mon:
        model(x)
    assert torch.equal(mon.counts()[3], c[0])


def test_refusals():
    model, _, _ = ms_model("lif", (144, 192), False)
    x = harness.prepare_chunk(synth_voxel(2, 10, 144, 192, seed=5)).to(DEV)
    mon = FiringRateMonitor(model)
    with mon:
        with pytest.raises((hip.SdfError, RuntimeError), match="forward_replicas"):
            model.forward_replicas(x)
        # the refusal comes before anything is packed: with no engine yet, a capture must not see the weight kernels and host copies
        model.invalidate_engine()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with pytest.raises((hip.SdfError, RuntimeError), match="graph capture"):
                with torch.cuda.graph(g, stream=s):
                    model(x[:1])
        torch.cuda.synchronize()
        assert model._engine is None, "the refused forward packed the engine under capture"
        try:
            model.train()
            with pytest.raises((hip.SdfError, RuntimeError), match="training mode"):
                model(x[:1])
        finally:
            model.eval()
    assert mon.forwards == 0
    model.forward_replicas(x)                                                   # disabled: as before
    cfg = config("lif", (144, 192))
    cfg.setdefault("loader", {})["crop"] = None
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    cfg["vis"] = {"monitor_fr": True}
    with pytest.raises((hip.SdfError, RuntimeError), match="monitor_fr"):
        harness.evaluate_stream(model, [], cfg, device=DEV)
    from sdformerflow_amd.STSwinNet.STSwinNet import STTFlowNet
    ann = STTFlowNet.__new__(STTFlowNet)                                        # (the class is enough: it is refused by type)
    with pytest.raises((hip.SdfError, RuntimeError), match="spiking model"):
        FiringRateMonitor(ann)
