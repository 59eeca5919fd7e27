"""Eval-mode forward of a GLIF model (engine_glif.GLIFFlowEngine): the statement of tests/test_replay_gpu.py `check` for the one
neuron type that has no fused kernel, and the entry points that sit on the eval plan.

Model: the 3-encoder MS model of test_replay_gpu's `build("glif", size, en4=False)` with the synthetic state and the gate logits
redrawn (glif_replay.redraw_gate_logits: with the synthetic default, all logits -0.1, 23 of the 78 neuron calls of the forward never fire).

Replay parity, per configuration: every taped neuron call is a delta-consistent execution of the reference recurrence on the
pre-activation the oracle forms from the GPU's own upstream spikes (0 unexplained decisions; glif_replay.glif_delta_consistent),
at most 2e-5 of the decisions are ambiguous, and the flows equal the replayed flows within FLOW_TOL of max |flow|.
delta = glif_replay.DELTA_ULPS ulps of max(rms(x), th); the ulps the departures actually needed are printed here and recorded beside
that constant (measured on the MI355X: 2.20 at B = 1, 2.75 at B = 2)."""
import copy
import functools

import pytest
import torch

import glif_replay
import replay
import test_replay_gpu as R
from oracle import sdformer_oracle as O
from sdformerflow_amd import harness, hip, train
from sdformerflow_amd.loss.flow_supervised import AEE
from sdformerflow_amd.monitor import FiringRateMonitor, neuron_call_names
from sdformerflow_amd.synthetic import synth_label, synth_voxel
from test_evaluate_stream_gpu import check_against, tuples

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {"B1": ((144, 192), 1, 77), "B2": ((144, 144), 2, 78)}           # name -> (size, batch, voxel seed)


@functools.lru_cache(maxsize=None)
def model_of(size):
    return glif_replay.build(size)


@functools.lru_cache(maxsize=None)
def replayed(name):
    """One taped forward and its oracle replay per configuration, shared by the tests below and left unchanged."""
    size, B, seed = CONFIGS[name]
    model, sd, ocfg = model_of(size)
    chunk = harness.prepare_chunk(synth_voxel(B, 10, size[0], size[1], seed=seed))
    flows, ref, report, tape = glif_replay.run(model.eval_engine(), chunk.to(DEV), lambda: O.forward_flownet(chunk, sd, ocfg))
    return {"model": model, "sd": sd, "chunk": chunk, "flows": flows, "ref": ref, "report": report, "tape": tape}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_free_running_forward_is_a_delta_consistent_execution_of_the_reference(name):
    r = replayed(name)
    model, report, flows = r["model"], r["report"], r["flows"]
    summ = replay.summarise(report)
    rates = [x["rate"] for x in report if x["forced"]]
    print(f"glif {name} {CONFIGS[name]}: {summ}; rates {min(rates):.3f} .. {max(rates):.3f}, mean {sum(rates) / len(rates):.3f}")
    for x in sorted((x for x in report if x["forced"]), key=lambda x: -x["needed_ulps"])[:4]:
        print(f"    {x['layer']:90s} flips {x['flips']:7d} ambiguous {x['ambiguous']:8d} of {x['n']:10d}  needed {x['needed_ulps']:.2f} ulps")
    assert summ["layers_forced"] == 78 and summ["layers_free"] == 0, summ      # every call the oracle's forward makes is on the tape
    assert min(rates) > 0.0, "a silent neuron call exercises nothing behind it"
    assert summ["unexplained"] == 0, [x for x in report if x["forced"] and x["unexplained"]][:5]
    assert summ["ambiguous"] <= 2e-5 * summ["decisions"], summ
    devs = []
    for g, ref in zip(flows, r["ref"]):
        g = g.cpu()
        assert g.shape == ref.shape and torch.isfinite(g).all()
        devs.append(float((g - ref).abs().max() / ref.abs().max()))
    print(f"    flows vs replayed reference: max-abs-dev / max|flow| per scale {['%.1e' % d for d in devs]}")
    assert max(devs) <= R.FLOW_TOL, devs
    # the plain forward is bit-equal to the taped one, and a second one to the first
    x = r["chunk"].to(DEV)
    plain, again = model(x)["flow"], model(x)["flow"]
    assert all(torch.equal(a, b) for a, b in zip(plain, flows)), "the untaped forward differs from the taped one"
    assert all(torch.equal(a, b) for a, b in zip(plain, again))


def test_entry_points():
    size, B, _ = CONFIGS["B2"]
    model, _, _ = model_of(size)
    with pytest.raises(hip.SdfError, match="no fused kernel"):
        model.engine()
    x = harness.prepare_chunk(synth_voxel(3, 10, size[0], size[1], seed=301)).to(DEV)
    out = model(x[:2])
    assert out["attn"] is None and len(out["flow"]) == 3
    assert all(f.shape == (2, 2) + size and f.dtype == torch.float32 and torch.isfinite(f).all() for f in out["flow"])
    with pytest.raises(NotImplementedError, match="log=True is not built"):
        model(x[:1], log=True)
    rep = model.forward_replicas(x)["flow"]
    assert len(rep) == 3 and rep[-1].shape == (3, 2) + size
    for i in range(3):
        one = model(x[i:i + 1])["flow"]
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(rep, one)), i
    assert not torch.equal(rep[-1][0], rep[-1][1])


def eval_config(size):
    import yaml
    cfg = yaml.safe_load(open(R.CFG))
    cfg["loader"] = dict(cfg["loader"], crop=list(size), polarity=True)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    return cfg


def test_harness_evaluate_and_the_graph_captured_stream():
    size, _, _ = CONFIGS["B2"]
    model, _, _ = model_of(size)
    cfg = eval_config(size)
    samples = tuples(4, size, seed0=310)
    res = harness.evaluate(model, samples[:2], cfg, device=DEV)
    want = 0.0
    for vox, mask, label in samples[:2]:
        with torch.no_grad():
            flow = model(harness.prepare_chunk(vox).to(DEV))["flow"][-1]
        want += float(AEE(flow, label.to(DEV), mask.to(DEV).unsqueeze(1).float(), 1)()[0][0]) / 2
    print("evaluate", res, "AEE of the model's own flows", want)
    assert want > 0 and abs(res["AEE"] - want) <= 1e-6 * want                  # (the bound of tests/test_harness.py for this identity)
    ref = harness.evaluate(model, samples, cfg, device=DEV)
    got = harness.evaluate_stream(model, samples, cfg, device=DEV, replicas=2, streams=2)
    print("evaluate_stream", got, "evaluate", ref)
    check_against(got, ref)                                                     # the same dict, to the summation orders of the two loops


def test_train_then_eval_runs_on_repacked_tables_and_planes():
    size, B = CONFIGS["B2"][0], 1
    model = copy.deepcopy(model_of(size)[0])                                    # (its own: the step changes the weights)
    model.invalidate_engine()
    chunk = harness.prepare_chunk(synth_voxel(B, 10, size[0], size[1], seed=1234 + 4)).to(DEV)
    label, mask = synth_label(B, *size)
    before = [f.clone() for f in model(chunk)["flow"]]
    tab0 = model.eval_engine().stages[0][0].sn_q.tab.clone()
    model.train()
    for m in model.modules():
        if hasattr(m, "drop_path_rate"):
            m.drop_path_rate = 0.0
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    loss = train.train_step(model, opt, chunk, label.to(DEV), mask.to(DEV), buckets=train.GradientBuckets(model.parameters()))
    assert torch.isfinite(loss).all()
    model.eval()
    after = model(chunk)["flow"]
    assert not any(torch.equal(a, b) for a, b in zip(after, before))
    assert not torch.equal(model.eval_engine().stages[0][0].sn_q.tab, tab0)
    fresh = copy.deepcopy(model_of(size)[0])
    fresh.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(fresh(chunk)["flow"], after))


def test_firing_rate_monitor_counts_every_call():
    r = replayed("B1")
    model, sd, tape, x = r["model"], r["sd"], r["tape"], r["chunk"].to(DEV)
    with FiringRateMonitor(model) as mon:
        flows = model(x)["flow"]
    assert mon.names == neuron_call_names(model) and len(mon.names) == 88 and mon.forwards == 1
    assert all(torch.equal(a, b) for a, b in zip(flows, r["flows"]))
    counts = mon.counts()[0].cpu()
    checked = 0
    for i, name in enumerate(mon.names):
        if name + "." in tape:
            t, layout = tape[name + "."]
            t_dim = 0 if layout == "flat" else 1
            want = t.transpose(0, t_dim).flatten(1).sum(1, dtype=torch.int64).cpu()
        else:
            # the dead attention score: the oracle's forward only runs it where scores are asked for, so the expected count is the
            # oracle's neuron on the gated, head-scrambled tensor formed from the taped k and gate spikes (0 / 1 inputs: exact)
            assert name.endswith("attn.attn_sn.spiking_neuron"), name
            p = name[:-len("attn_sn.spiking_neuron")]
            k, a = tape[p + "sn_k.spiking_neuron."][0].cpu(), tape[p + "sn2_q.spiking_neuron."][0].cpu()
            Tq, rows, Cc = k.shape
            nH, N1 = a.shape[-1], 81
            e = (k * a.repeat_interleave(Cc // nH, dim=-1)).float()
            z = e.reshape(rows // N1, nH, Tq, N1, Cc // nH).permute(2, 0, 3, 1, 4).reshape(Tq, rows // N1, N1, Cc)
            want = O.glif_multistep(z, sd, name + ".").flatten(1).sum(1).to(torch.int64)
        T = want.numel()
        assert torch.equal(counts[i, :T], want) and int(counts[i, T:].sum()) == 0, name
        assert int(want.sum()) > 0, name
        checked += 1
    assert checked == 88


def test_launches_of_one_forward():
    r = replayed("B1")
    model, x = r["model"], r["chunk"].to(DEV)
    with hip.launch_log() as log:
        model(x)
    torch.cuda.synchronize()
    names = [row[0] for row in log.rows]
    glif = [n for n in names if "glif_neuron_kernel<" in n]
    gate = [n for n in names if "qk_gate_glif_kernel<" in n]
    # 78 neuron calls of the forward, the 10 token gates among them in the gate kernel; the decoders launch once per source
    assert len(gate) == 10 and len(glif) >= 68, (len(gate), len(glif))
    other = [n for n in names if "glif_neuron_kernel<" not in n]
    for pattern in ("neuron_kernel<", "qk_gate_kernel(", "plif_fwd_kernel", "neuron_multi_kernel<", "head_conv"):
        assert not any(pattern in n for n in other), pattern
