"""Firing rates at the streamed rate: monitor.ReplicaFiringRateMonitor counts every sample of `model.forward_replicas(x[R])` - eagerly,
under graph capture into a count block, and through harness.evaluate_stream(..., monitor=) - and must give, integer for integer, the
stacked counts of R separate `model(x[i:i+1])` under FiringRateMonitor (whose own exactness against the oracle replay is
tests/test_firing_rate_gpu.py's).  The inputs differ per sample and the tests assert that their count rows differ: a wrong split of a
record between the samples would move spikes from one row to another."""
import csv

import pytest
import torch

from sdformerflow_amd import harness, hip
from sdformerflow_amd.monitor import FiringRateMonitor, MembraneMonitor, ReplicaFiringRateMonitor
from sdformerflow_amd.synthetic import synth_label, synth_voxel
from test_firing_rate_gpu import config, ms_model, sew_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def inputs(R, size, seed):
    """R different samples (R, bins, 2, H, W) on the device."""
    return torch.cat([harness.prepare_chunk(synth_voxel(1, 10, *size, seed=seed + 17 * i)) for i in range(R)], 0).to(DEV)


def one_by_one(model, x):
    """The reference of every test: R separate monitored batch-1 forwards -> (counts (R, calls, Tmax), elements, last-level flows)."""
    mon = FiringRateMonitor(model)
    with mon:
        flows = [model(x[i:i + 1])["flow"][-1] for i in range(x.shape[0])]
    return mon.counts().clone(), mon.elements, torch.cat(flows, 0)


def rows_differ(counts):
    return all(not torch.equal(counts[i], counts[j]) for i in range(counts.shape[0]) for j in range(i))


def check_replicas(model, x):
    want, elements, flow1 = one_by_one(model, x)
    assert rows_differ(want), "every sample has the same counts: the test would not see a wrong split"
    plain = model.forward_replicas(x)["flow"]
    mon = ReplicaFiringRateMonitor(model)
    with mon:
        monitored = model.forward_replicas(x)["flow"]
    assert not mon.enabled and model._fr_monitor is None and mon.forwards == x.shape[0]
    got = mon.counts()
    assert got.shape == want.shape and got.dtype == torch.int64
    bad = [(r, mon.names[i], got[r, i].tolist(), want[r, i].tolist())
           for r, i in (got != want).any(-1).nonzero().tolist()]
    assert not bad, (len(bad), bad[:4])
    assert mon.elements == elements
    assert all(torch.equal(a, b) for a, b in zip(monitored, plain)), "the monitored replica forward differs from the plain one"
    assert torch.equal(monitored[-1], flow1)
    return mon, want


def test_lif_three_replicas_equal_three_monitored_forwards():
    model, _, _ = ms_model("lif", (144, 192), False)
    mon, want = check_replicas(model, inputs(3, (144, 192), 300))
    # reading side: one record set per sample, in sample order
    recs = mon.records
    assert len(recs) == 3 and len(recs[0]) == len(mon.names)
    for r in range(3):
        for i in (0, 7, len(mon.names) - 1):
            T = recs[r][i].numel()
            assert torch.equal(recs[r][i], (want[r, i, :T].cpu().double() / mon.elements[i]).float())
    assert 0.0 < mon.mean() < 1.0 and list(mon.rates()) == mon.names


def test_one_count_launch_per_record_serves_all_samples():
    """The replica launch sequence counts every record with ONE launch of the per-sample kernel; the one-by-one route with the
    single-sample kernel, once per sample (150 x 200: the replica sequence is begun, meets the odd window count at a later stage and
    is abandoned - its rows are zeroed - so fewer than a full set of per-sample launches come first)."""
    for size, single in (((144, 192), 0), ((150, 200), 3)):
        model, _, _ = ms_model("lif", size, False)
        x = inputs(3, size, 350)
        mon = ReplicaFiringRateMonitor(model)
        with mon, hip.launch_log() as log:
            model.forward_replicas(x)
        names = [r[0] for r in log.rows if "spike_count" in r[0]]
        seg = sum("spike_count_seg_" in n for n in names)
        assert (seg == len(mon.names)) if single == 0 else (seg < len(mon.names)), (size, seg)
        assert len(names) - seg == single * len(mon.names), size


def test_psn_two_replicas_equal_two_monitored_forwards():
    """The PSN token gates fire at intermediate rates that differ between steps and samples: the recomputed gate's per-sample layout."""
    model, _, _ = ms_model("psn", (144, 192), False)
    mon, want = check_replicas(model, inputs(2, (144, 192), 400))
    gates = [i for i, n in enumerate(mon.names) if "sn2_q" in n]
    rates = [[float(want[r, i, :2].sum()) / (2 * mon.elements[i]) for i in gates] for r in range(2)]
    assert any(0.05 < g < 0.95 for g in rates[0]), rates
    assert rates[0] != rates[1]


def test_a_single_sample_and_a_later_group_append_rows():
    model, _, _ = ms_model("lif", (144, 192), False)
    x = inputs(3, (144, 192), 500)
    want, _, _ = one_by_one(model, x)
    mon = ReplicaFiringRateMonitor(model, forwards=1)                        # (the table grows: 1 -> 3 rows)
    with mon:
        model(x[:1])
        model.forward_replicas(x[1:])
    assert mon.forwards == 3 and torch.equal(mon.counts(), want)


def test_captured_into_a_block_and_replayed_on_fresh_inputs():
    model, _, _ = ms_model("lif", (144, 192), False)
    xs = [inputs(3, (144, 192), 600), inputs(3, (144, 192), 700)]
    wants = [one_by_one(model, x)[0] for x in xs]
    mon = ReplicaFiringRateMonitor(model)
    static = xs[0].clone()
    block = torch.zeros((3, len(mon.names), mon.Tmax), dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    with mon, torch.cuda.stream(s):
        # a capture without a block is refused before the engine is packed
        model.invalidate_engine()
        g = torch.cuda.CUDAGraph()
        with pytest.raises((hip.SdfError, RuntimeError), match="count block"):
            with torch.cuda.graph(g, stream=s):
                model.forward_replicas(static)
        torch.cuda.synchronize()
        assert model._engine is None, "the refused forward packed the engine under capture"
        assert mon.forwards == 0
        with mon.into(block):
            for _ in range(2):
                model.forward_replicas(static)                                # (workspaces and plan caches of this stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            block.zero_()
            with mon.into(block):
                flow = model.forward_replicas(static)["flow"][-1]
        assert mon.forwards == 0                                              # filling a block leaves the table alone
        for k, (x, want) in enumerate(zip(xs[::-1], wants[::-1])):            # fresh inputs, the capture's own last
            static.copy_(x)
            g.replay()
            assert torch.equal(block, want), f"replay {k}"
            mon.take(block, first=3 * k)
        torch.cuda.synchronize()
    assert mon.forwards == 6 and torch.equal(mon.counts(), torch.cat(wants[::-1], 0))
    assert torch.equal(flow, model.forward_replicas(xs[0])["flow"][-1])


def test_one_by_one_route_at_an_odd_window_count():
    """150 x 200: odd window counts, forward_replicas serves the samples one by one - and so does the monitor, sample i into row i."""
    model, _, _ = ms_model("lif", (150, 200), False)
    check_replicas(model, inputs(2, (150, 200), 800))


def test_one_by_one_route_of_the_sew_family():
    model, _, _ = sew_model("lif")
    mon, _ = check_replicas(model, inputs(2, (144, 192), 900))
    assert len(mon.names) == 75


def stream_case():
    model, _, _ = ms_model("lif", (144, 192), False)
    cfg = config("lif", (144, 192))
    cfg.setdefault("loader", {})["crop"] = None
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    label, mask = synth_label(1, 144, 192)
    samples = [(synth_voxel(1, 10, 144, 192, seed=40 + 3 * i), mask, label) for i in range(5)]
    return model, cfg, samples


@pytest.fixture(scope="module")
def eager_loop():
    """harness.evaluate with FiringRateMonitor over the five samples: computed once, shared, left unchanged."""
    model, cfg, samples = stream_case()
    mon = FiringRateMonitor(model)
    harness.evaluate(model, samples, dict(cfg, vis={"monitor_fr": True}), device=DEV, monitor=mon)
    return mon.counts().clone(), mon.elements


@pytest.mark.parametrize("graphs", [True, False])
def test_evaluate_stream_with_the_monitor(graphs, eager_loop, tmp_path):
    """Five samples at replicas = 2 on two streams: groups of 2, 2 and 1 - the n = 1 graph is covered."""
    model, cfg, samples = stream_case()
    want, elements = eager_loop
    assert rows_differ(want)
    assert [n for _, _, n in harness.stream_plan(5, 2, 2)] == [2, 2, 1]
    plain = harness.evaluate_stream(model, samples, cfg, device=DEV, replicas=2, streams=2, graphs=graphs)
    mon = ReplicaFiringRateMonitor(model)
    got = harness.evaluate_stream(model, samples, cfg, device=DEV, replicas=2, streams=2, graphs=graphs, monitor=mon)
    assert got == plain
    assert not mon.enabled and model._fr_monitor is None and mon.forwards == 5
    assert torch.equal(mon.counts(), want) and mon.elements == elements
    path = tmp_path / "firing_rate.csv"
    mon.to_csv(path)
    rows = list(csv.reader(open(path)))
    assert len(rows) == 5 * len(mon.names)
    assert rows[0][:2] == ["0", mon.names[0]] and rows[-1][:2] == ["4", mon.names[-1]]


def test_an_evaluator_keeps_its_graphs_over_runs_and_resets(eager_loop):
    """The step counts and denominators of a captured sequence serve every replay: after monitor.reset(), and appended behind the
    rows of an earlier run (the table, sized for 5, is grown before the second run's streams start)."""
    model, cfg, samples = stream_case()
    want, elements = eager_loop
    mon = ReplicaFiringRateMonitor(model, forwards=1)
    ev = harness.StreamEvaluator(model, cfg, DEV, replicas=2, streams=2, graphs=True, monitor=mon)
    first = ev.run(samples)
    mon.reset()
    assert mon.forwards == 0
    assert ev.run(samples) == first and torch.equal(mon.counts(), want)
    assert ev.run(iter(samples)) == first                                     # (an iterable without len())
    assert mon.forwards == 10 and torch.equal(mon.counts(), torch.cat([want, want], 0)) and mon.elements == elements
    # 70 samples of unknown number: the table is sized for 64 and grows on the way, behind a wait for both streams
    mon.reset()
    ev.run(s for s in samples * 14)
    assert mon.forwards == 70 and torch.equal(mon.counts(), torch.cat([want] * 14, 0))


def test_refusals():
    model, cfg, samples = stream_case()
    x = inputs(2, (144, 192), 5)
    mon = ReplicaFiringRateMonitor(model)
    with mon:
        with pytest.raises((hip.SdfError, RuntimeError), match="FiringRateMonitor"):
            model(x)                                                          # a reference batch couples its samples
        with pytest.raises(RuntimeError, match="one monitor at a time"):
            ReplicaFiringRateMonitor(model).enable()                          # two monitors on one model
        with pytest.raises(RuntimeError, match="one monitor at a time"):
            FiringRateMonitor(model).enable()
        try:
            model.train()
            with pytest.raises((hip.SdfError, RuntimeError), match="training mode"):
                model(x[:1])
            with pytest.raises((hip.SdfError, RuntimeError), match="model.eval"):
                model.forward_replicas(x)
        finally:
            model.eval()
        with pytest.raises(hip.SdfError, match="count block"):
            with mon.into(torch.zeros((3, len(mon.names), mon.Tmax), dtype=torch.int64, device=DEV)):
                model.forward_replicas(x)                                     # a block of 3 samples for a forward of 2
        with pytest.raises(hip.SdfError, match="count block"):
            mon.into(torch.zeros((2, len(mon.names), mon.Tmax), dtype=torch.int32, device=DEV)).__enter__()
    assert mon.forwards == 0 and int(mon.counts().sum()) == 0
    with pytest.raises(hip.SdfError, match="no forward has filled"):
        mon.take(torch.zeros((2, len(mon.names), mon.Tmax), dtype=torch.int64, device=DEV))
    for other in (FiringRateMonitor(model), MembraneMonitor(model)):
        with pytest.raises(TypeError, match="ReplicaFiringRateMonitor"):
            harness.evaluate_stream(model, samples, cfg, device=DEV, monitor=other)
    with pytest.raises(ValueError, match="another model"):
        harness.evaluate_stream(model, samples, cfg, device=DEV, monitor=ReplicaFiringRateMonitor(ms_model("psn", (144, 192), False)[0]))
    with pytest.raises((hip.SdfError, RuntimeError), match="monitor_fr"):
        harness.evaluate_stream(model, samples, dict(cfg, vis={"monitor_fr": True}), device=DEV)
    assert model._fr_monitor is None
