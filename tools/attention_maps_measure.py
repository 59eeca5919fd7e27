#!/usr/bin/env python3
"""Time of a `log=True` forward next to the plain one on one MI355X -> <dir>/attention_maps_timing.txt:

  the config-3 ANN model (STTFlowNet, 1 x 20 x 288 x 384) and the SEW model (SpikingformerFlowNet, lif, 1 x 10 x 2 x 288 x 384), single
  stream, eager: median (min, max) of 20 forwards with HIP events, plain and with log=True; the bytes of the returned maps; the
  win_attn_scores_kernel launches of one log=True forward from hip.launch_log.

Usage: python tools/attention_maps_measure.py [dir = profiles]"""
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from firing_rate_measure import DEV, build, forward_ms                                                 # noqa: E402
from sdformerflow_amd import harness, hip                                                              # noqa: E402
from sdformerflow_amd.STSwinNet import STSwinNet                                                       # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet                      # noqa: E402
from sdformerflow_amd.synthetic import synth_state_dict, synth_voxel                                   # noqa: E402

SIZE = (288, 384)
DERIVED = ("relative_position_index", "relative_coords_table", "num_batches_tracked")


def ann_model():
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_STT_voxel.yml")))
    net = STSwinNet.STTFlowNet(dict(cfg["model"], spiking_neuron=None), dict(cfg["swin_transformer"], input_size=list(SIZE)))
    net.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith(DERIVED)}), strict=False)
    net.norm_input = False
    return net.to(DEV).eval()


def measure(what, plain, logged, lines):
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f})"
    t_plain, t_log = forward_ms(plain), forward_ms(logged)
    with hip.launch_log() as log:
        maps = logged()["attn"]
    torch.cuda.synchronize()
    rows = [r for r in log.rows if "win_attn_scores_kernel" in r[0]]
    mb = [m.numel() * 4 / 1e6 for m in maps]
    lines.append(f"{what}, single stream, eager, median (min, max) of 20 forwards in ms: plain {fmt(t_plain)}; log=True {fmt(t_log)}; "
                 f"maps {[tuple(m.shape) for m in maps]} = {', '.join(f'{v:.1f}' for v in mb)} MB; win_attn_scores_kernel launches "
                 f"{', '.join(f'{r[4]:.1f} us' for r in rows)} ({', '.join(f'{v / r[4]:.2f} TB/s' for v, r in zip(mb, rows))} of stored map)")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    lines = []
    net = ann_model()
    vox = synth_voxel(1, 20, *SIZE, seed=1237).to(DEV)
    measure("STTFlowNet (config 3) at 1 x 20 x 288 x 384", lambda: net(vox, None), lambda: net(vox, None, log=True), lines)
    del net
    torch.cuda.empty_cache()
    sew = build(SpikingformerFlowNet, "lif", SIZE, True)
    x = harness.prepare_chunk(synth_voxel(1, 10, *SIZE, seed=1235)).to(DEV)
    measure("SpikingformerFlowNet (SEW, lif) at 1 x 10 x 2 x 288 x 384", lambda: sew(x), lambda: sew(x, log=True), lines)
    with open(os.path.join(out, "attention_maps_timing.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
