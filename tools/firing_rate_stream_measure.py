#!/usr/bin/env python3
"""Firing rates at the streamed rate, measured on one MI355X: the en4 model, lif and psn, at 288 x 384, one
process, three schemes ALTERNATED repetition by repetition over the same samples on the device:

  stream          harness.evaluate_stream(replicas=R, streams=2, graphs=True), no monitor
  stream+monitor  the same with monitor=ReplicaFiringRateMonitor(model): per-sample counts from the captured sequence
  eager loop      harness.evaluate with vis.monitor_fr and a FiringRateMonitor: single eager forwards - the only route to the rates
                  before the replica monitor

per scheme: samples/s as median (min, max) over the repetitions (host clock around the call, which ends synchronised), and the peak
of torch's allocated bytes above what was allocated before the scheme's first run (that run captures the graphs).  R is the largest
of 10, 8, 5, 4, 2 whose monitored graphs fit.  Then the device time of the per-sample count launches of ONE eager R-sample sequence
(hip.launch_log), and the ratio the README may quote: monitored stream / eager loop, against the run-to-run range of the two.

Usage: python tools/firing_rate_stream_measure.py [dir = profiles] [samples = 40] [repetitions = 7]"""
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdformerflow_amd import harness, hip                                                              # noqa: E402
from sdformerflow_amd.monitor import FiringRateMonitor, ReplicaFiringRateMonitor                       # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4               # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel                      # noqa: E402

DEV = "cuda:0"
CFG = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
SIZE = (288, 384)


def build(kind):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=10)
    cfg["model"]["num_bins"] = 10
    cfg["swin_transformer"].update(input_size=list(SIZE), window_size=[2, 9, 9])
    model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("relative_position_index")}
    model.load_state_dict(synth_state_dict(shapes), strict=False)
    cfg.setdefault("loader", {})["crop"] = None
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    cfg["vis"] = {}
    return model.eval().to(DEV), cfg


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def first_run(fn):
    """The scheme's first run (plan caches, workspaces, graph capture): -> peak allocated bytes above the level before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(kind, n, reps, lines):
    model, cfg = build(kind)
    label, mask = synth_label(1, *SIZE)
    samples = [(synth_voxel(1, 10, *SIZE, seed=100 + i).to(DEV), mask.to(DEV), label.to(DEV)) for i in range(n)]
    cfg_fr = dict(cfg, vis={"monitor_fr": True})
    eager_mon = FiringRateMonitor(model, forwards=n)

    def eager():
        eager_mon.reset()
        harness.evaluate(model, samples, cfg_fr, device=DEV, monitor=eager_mon)
    peaks = {"eager loop": first_run(eager)}
    R, plain, monitored, rep_mon = None, None, None, None
    for r in (10, 8, 5, 4, 2):
        try:
            rep_mon = ReplicaFiringRateMonitor(model, forwards=n)
            monitored = harness.StreamEvaluator(model, cfg, DEV, replicas=r, streams=2, graphs=True, monitor=rep_mon)
            peaks["stream+monitor"] = first_run(lambda: monitored.run(samples))
            R = r
            break
        except torch.OutOfMemoryError:
            monitored = rep_mon = None
            torch.cuda.empty_cache()
            lines.append(f"en4 {kind}: the monitored graphs of replicas = {r} on 2 streams do not fit")
    if R is None:
        raise SystemExit("no replica count fits")
    assert torch.equal(rep_mon.counts(), eager_mon.counts()), "the streamed counts differ from the eager loop's"
    plain = harness.StreamEvaluator(model, cfg, DEV, replicas=R, streams=2, graphs=True)
    peaks["stream"] = first_run(lambda: plain.run(samples))

    def stream_monitored():
        rep_mon.reset()
        monitored.run(samples)
    schemes = {"stream": lambda: plain.run(samples), "stream+monitor": stream_monitored, "eager loop": eager}
    rates = {k: [] for k in schemes}
    for _ in range(reps):                                          # alternated: drift of clocks and temperature hits all three alike
        for k, fn in schemes.items():
            rates[k].append(n / timed(fn))
    lines.append(f"en4 {kind}, {SIZE[0]} x {SIZE[1]}, {n} samples on the device, replicas = {R} (the largest of 10, 8, 5, 4, 2 whose "
                 f"monitored graphs fit), 2 streams, {reps} repetitions alternated; samples/s median (min, max), peak allocated of the first run:")
    med = {}
    for k, v in rates.items():
        v = sorted(v)
        med[k] = v[len(v) // 2]
        lines.append(f"  {k:15s} {med[k]:8.1f} ({v[0]:.1f}, {v[-1]:.1f}) samples/s   peak +{peaks[k] / 2 ** 30:.2f} GiB")
    ratio = med["stream+monitor"] / med["eager loop"]
    lo = min(rates["stream+monitor"]) / max(rates["eager loop"])
    hi = max(rates["stream+monitor"]) / min(rates["eager loop"])
    verdict = "above" if lo > 1.0 else "NOT above"
    lines.append(f"  monitored stream / eager monitored loop = {ratio:.2f} (worst pairing of the repetitions {lo:.2f}, best {hi:.2f}): "
                 f"{verdict} the run-to-run range of the two; monitored stream / plain stream = {med['stream+monitor'] / med['stream']:.2f}")
    lines.append(f"  reserved by the allocator at the end (both evaluators' graph pools alive): {torch.cuda.memory_reserved() / 2 ** 30:.2f} GiB")
    # one eager R-sample sequence: its per-sample count launches
    x = torch.cat([harness.prepare_chunk(s[0]) for s in samples[:R]], 0)
    probe = ReplicaFiringRateMonitor(model, forwards=R)
    with probe:
        model.forward_replicas(x)
        with hip.launch_log() as log:
            model.forward_replicas(x)
    rows = [r for r in log.rows if "spike_count" in r[0]]
    seg = [r for r in rows if "spike_count_seg_" in r[0]]
    lines.append(f"  count launches of one eager R = {R} sequence: {len(rows)}, {len(seg)} of them per-sample launches "
                 f"({sum('seg_run' in r[0] for r in seg)} dense, {sum('seg_rows' in r[0] for r in seg)} strided), {sum(r[4] for r in seg):.1f} us "
                 f"in all for {R} samples (event-timed one by one); every launch of the sequence: {len(log.rows)}, {sum(r[4] for r in log.rows) / 1e3:.2f} ms")
    del plain, monitored
    torch.cuda.empty_cache()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    reps = max(int(sys.argv[3]) if len(sys.argv) > 3 else 7, 5)
    os.makedirs(out, exist_ok=True)
    lines = []
    for kind in ("lif", "psn"):
        measure(kind, n, reps, lines)
    with open(os.path.join(out, "firing_rate_stream_timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
