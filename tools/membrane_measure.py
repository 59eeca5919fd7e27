"""Membrane monitor: one monitored forward against one plain forward of the en4 lif model at 288 x 384 (and the unfused plan alone), wall
clock, and the peak allocated memory with keep=() - the figures of DESIGN.md section 7 / profiles/membrane_monitor_timing.txt.

usage: python tools/membrane_measure.py    (one MI355X)"""
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sdformerflow_amd import harness  # noqa: E402
from sdformerflow_amd.monitor import MembraneMonitor  # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4  # noqa: E402
from sdformerflow_amd.synthetic import synth_state_dict, synth_voxel  # noqa: E402

cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif", num_steps=10)
cfg["model"]["num_bins"] = 10
cfg["swin_transformer"].update(input_size=[288, 384], window_size=[2, 9, 9])
model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
model = model.eval().to("cuda:0")
x = harness.prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1235)).to("cuda:0")


def timed(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20


plain_ms, plain_mb = timed(lambda: model(x))
unf = model.unfused_engine()
unf_ms, unf_mb = timed(lambda: unf.forward(x))
mon = MembraneMonitor(model, forwards=64)
with mon:
    mon_ms, mon_mb = timed(lambda: model(x))
lines = [f"en4, lif, 288 x 384, batch 1, 10 forwards after 3 warm-up, wall clock with one synchronisation at the end",
         f"plain fused forward          {plain_ms:8.2f} ms   peak allocated {plain_mb:8.1f} MiB",
         f"plain unfused forward        {unf_ms:8.2f} ms   peak allocated {unf_mb:8.1f} MiB",
         f"monitored forward, keep=()   {mon_ms:8.2f} ms   peak allocated {mon_mb:8.1f} MiB   ({len(mon.names)} calls, {mon.forwards} forwards recorded)"]
print("\n".join(lines))
