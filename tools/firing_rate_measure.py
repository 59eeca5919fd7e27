#!/usr/bin/env python3
"""Measurements of the firing-rate monitor on one MI355X.

  <dir>/firing_rate_vs_fixture.txt  per-call |rate of the free-running HIP forward - the reference's own run| for the four fixture
                                    forwards (en4 and SEW, lif and psn)
  <dir>/firing_rate_timing.txt      the count kernels with hip.launch_log (the largest record, en4 patch_embed.head.sn, once over ONE
                                    buffer - which the 256 MiB Infinity Cache holds between launches - and once rotating over four, 425
                                    MB, which it does not; the q half of a stacked q | k buffer), and the plain, monitored and taped
                                    forward of config 2 with HIP events

Usage: python tools/firing_rate_measure.py [dir = profiles]"""
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdformerflow_amd import harness, hip                                                              # noqa: E402
from sdformerflow_amd.monitor import FiringRateMonitor                                                 # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4, SpikingformerFlowNet   # noqa: E402
from sdformerflow_amd.synthetic import synth_state_dict, synth_voxel                                   # noqa: E402

DEV = "cuda:0"
CFG = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")


def build(cls, kind, size, en3):
    """The model of a fixture forward: the shipped config with the fixture's neuron, size and depth, the synthetic state."""
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=10)
    cfg["model"]["num_bins"] = 10
    cfg["swin_transformer"].update(input_size=list(size), window_size=[2, 9, 9])
    if en3:
        cfg["swin_transformer"].update(swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    model = cls(cfg["model"].copy(), cfg["swin_transformer"].copy())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith("relative_position_index")}
    model.load_state_dict(synth_state_dict(shapes), strict=False)
    return model.eval().to(DEV)


def deviations(model, chunk, fixture, kind, lines):
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    mon = FiringRateMonitor(model)
    with mon:
        model(chunk.to(DEV))
    names, ref = [str(n) for n in g[f"{kind}_rate_names"]], g[f"{kind}_rates"].astype(np.float64)
    assert mon.names == names
    got = np.array([float(r.double().mean()) for r in mon.records[0]])
    dev = np.abs(got - ref)
    lines.append(f"# {fixture} {kind}: {len(names)} calls; max |gpu - fixture| {dev.max():.3e} at {names[int(dev.argmax())]}; "
                 f"mean of rates gpu {mon.mean():.6f} fixture {ref.mean():.6f} (dev {abs(mon.mean() - ref.mean()):.2e})")
    for n, a, b, d, el in zip(names, got, ref, dev, mon.elements):
        lines.append(f"{fixture[:-4]:15s} {kind} {n:95s} elements/step {el:9d} gpu {a:.6f} fixture {b:.6f} dev {d:.2e}")
    return float(dev.max())


def kernel_us(views, t_dim, launches):
    """Event-timed durations (hip.launch_log) of `launches` count launches, going round the views: (sorted us, workgroups)."""
    counts = torch.zeros(views[0].shape[t_dim], dtype=torch.int64, device=DEV)
    for v in views:
        hip.spike_count(v, t_dim, counts)
    us = []
    for i in range(launches):
        with hip.launch_log() as log:
            hip.spike_count(views[i % len(views)], t_dim, counts)
        us.append(log.rows[0][4])
    return sorted(us), log.rows[0][1]


def forward_ms(fn, n=20, warm=5):
    """(median, min, max) ms of n forwards, HIP events around each."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    lines, worst, en4_lif = [], [], None
    for kind in ("lif", "psn"):
        en4 = build(MS_SpikingformerFlowNet_en4, kind, (288, 384), False)
        en4_lif = en4_lif or en4
        worst.append(deviations(en4, harness.prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1235)), "end_to_end.npz", kind, lines))
        sew = build(SpikingformerFlowNet, kind, (144, 192), True)
        worst.append(deviations(sew, harness.prepare_chunk(synth_voxel(1, 10, 144, 192, seed=1234 + 7)), "sew_end_to_end.npz", kind, lines))
    lines.insert(0, f"# per-call |firing rate of the free-running HIP forward - reference fixture|, MI355X; overall max {max(worst):.3e}")
    with open(os.path.join(out, "firing_rate_vs_fixture.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(ln for ln in lines if ln.startswith("#")))

    tl = []
    torch.manual_seed(0)
    bufs = [(torch.rand((1, 10, 288, 384, 96), device=DEV) < 0.1).to(torch.uint8) for _ in range(4)]    # en4 patch_embed.head.sn: 106 MB each
    nbytes = bufs[0].numel()
    for what, views in (("ONE buffer, 20 launches (it stays in the 256 MiB Infinity Cache)", bufs[:1]),
                        ("four buffers in turn, 425 MB, 20 launches (each launch reads from HBM)", bufs)):
        us, wg = kernel_us(views, 1, 20)
        med = us[len(us) // 2]
        tl.append(f"spike_count_run_kernel on (1, 10, 288, 384, 96) u8 = {nbytes} bytes, {wg} workgroups, {what}: median {med:.1f} us "
                  f"(min {us[0]:.1f}, max {us[-1]:.1f}; event-timed by hip.launch_log) = {nbytes / med / 1e6:.2f} TB/s")
    del bufs
    qk = (torch.rand((69120, 192), device=DEV) < 0.1).to(torch.uint8)          # stage 0 of en4 at 288 x 384: 2 x 34 560 rows of q | k
    q = qk[:, :96].reshape(2, -1, 96)
    us, _ = kernel_us([q], 0, 10)
    tl.append(f"spike_count_rows_kernel on the q half of a ({qk.shape[0]}, 192) q|k buffer = {q.numel()} bytes: median {us[len(us) // 2]:.1f} us")

    model = en4_lif
    x = harness.prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1235)).to(DEV)
    plain = forward_ms(lambda: model(x))
    mon = FiringRateMonitor(model, forwards=64)
    with mon:
        monitored = forward_ms(lambda: model(x))
        with hip.launch_log() as log:
            model(x)
    rows = [r for r in log.rows if "spike_count" in r[0]]
    eng = model.engine()
    eng.tape = []
    try:
        taped = forward_ms(lambda: (eng.tape.clear(), model(x)))
    finally:
        eng.tape = None
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f})"
    tl.append("config 2 (en4 lif, 1 x 10 x 2 x 288 x 384), single stream, eager, median (min, max) of 20 forwards in ms: "
              f"plain {fmt(plain)}; monitored {fmt(monitored)}; parity tape {fmt(taped)}")
    tl.append(f"count launches in one monitored forward: {len(rows)} ({sum('run_kernel' in r[0] for r in rows)} contiguous, "
              f"{sum('rows_kernel' in r[0] for r in rows)} strided), {sum(r[4] for r in rows):.1f} us in all (event-timed one by one)")
    with open(os.path.join(out, "firing_rate_timing.txt"), "w") as f:
        f.write("\n".join(tl) + "\n")
    print("\n".join(tl))


if __name__ == "__main__":
    main()
