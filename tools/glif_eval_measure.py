#!/usr/bin/env python3
"""Timings of the unfused eval forward of a GLIF model on one MI355X -> <dir>/glif_eval_timing.txt:

  the en4 GLIF model at 1 x 10 x 2 x 288 x 384, single stream, eager: median (min, max) of 20 forwards with HIP events; beside it, in
  the same run, the en4 lif model's plain and parity-tape forwards; the per-kernel table of ONE GLIF forward from hip.launch_log; the
  general GLIF launch against the contiguous glif_fwd_kernel on the largest neuron call of that forward (patch_embed.head.sn).

The GLIF gate logits are redrawn as tests/glif_replay.py draws them (the synthetic default leaves 23 neuron calls silent).

Usage: python tools/glif_eval_measure.py [dir = profiles]"""
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from firing_rate_measure import DEV, build, forward_ms                                                 # noqa: E402
from sdformerflow_amd import harness, hip                                                              # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4               # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import GatedLIFNode                             # noqa: E402
from sdformerflow_amd.synthetic import synth_voxel                                                     # noqa: E402

LOGIT_RANGE = {"v_threshold": (-3.5, -2.0), "linear_decay": (-6.0, -4.0)}


def redraw_gate_logits(model, seed=5):
    nodes = {name for name, m in model.named_modules() if isinstance(m, GatedLIFNode)}
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            owner, _, leaf = name.rpartition(".")
            if owner in nodes:
                lo, hi = LOGIT_RANGE.get(leaf, (-1.0, 1.0))
                p.copy_((torch.rand(p.shape, generator=g) * (hi - lo) + lo).to(p.device))
    return model


def short(kernel):
    """Kernel name without its namespace and argument list."""
    name = kernel.replace("(anonymous namespace)::", "").replace("sdfmm::", "")
    return name.split("(")[0].replace("void ", "")


def kernel_us(fn, launches=10):
    fn()
    us = []
    for _ in range(launches):
        with hip.launch_log() as log:
            fn()
        us.append(log.rows[0][4])
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(out, exist_ok=True)
    x = harness.prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1235)).to(DEV)
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f}, {t[2]:.3f})"
    tl = []

    lif = build(MS_SpikingformerFlowNet_en4, "lif", (288, 384), False)
    plain = forward_ms(lambda: lif(x))
    eng = lif.engine()
    eng.tape = []
    try:
        taped = forward_ms(lambda: (eng.tape.clear(), lif(x)))
    finally:
        eng.tape = None
    del lif, eng
    torch.cuda.empty_cache()

    glif = redraw_gate_logits(build(MS_SpikingformerFlowNet_en4, "glif", (288, 384), False))
    t_glif = forward_ms(lambda: glif(x))
    tl.append("en4 at 1 x 10 x 2 x 288 x 384, single stream, eager, median (min, max) of 20 forwards in ms: "
              f"glif (unfused eval plan) {fmt(t_glif)}; lif plain {fmt(plain)}; lif parity tape {fmt(taped)}")
    with hip.launch_log() as log:
        glif(x)
    torch.cuda.synchronize()
    table = OrderedDict()
    for kernel, wgs, _, _, us in log.rows:
        n, t = table.get(short(kernel), (0, 0.0))
        table[short(kernel)] = (n + 1, t + us)
    total = sum(t for _, t in table.values())
    tl.append(f"one glif forward under hip.launch_log: {len(log.rows)} library launches, {total:.1f} us of kernel time (event-timed one by "
              "one; the library convolution of the head and torch's own kernels are not in the log)")
    for name, (n, t) in sorted(table.items(), key=lambda kv: -kv[1][1]):
        tl.append(f"    {name:60s} launches {n:4d}  us {t:9.1f}  share {100 * t / total:5.1f} %")

    # the general launch against the contiguous kernel on the forward's largest call: (10, 288 x 384 x 96) fp32 -> u8
    T, N = 10, 288 * 384 * 96
    tab = glif.eval_engine().head_sn.tab
    del glif
    torch.cuda.empty_cache()
    xs = torch.rand((T, N), device=DEV) - 0.3
    o = torch.empty((T, N), dtype=torch.uint8, device=DEV)
    nbytes = T * N * 5
    for what, fn in (("glif_neuron_kernel<10> (general launch, dense)", lambda: hip.glif_neuron_fwd(xs, o, T, 1, N, 0, N, 0, N, tab)),
                     ("glif_fwd_kernel<10, true> (contiguous)", lambda: hip.glif_fwd(xs, tab, torch.uint8))):
        med, lo, hi = kernel_us(fn)
        tl.append(f"{what} on (10, {N}) fp32 -> u8 = {nbytes} bytes: median {med:.1f} us (min {lo:.1f}, max {hi:.1f}) = "
                  f"{nbytes / med / 1e6:.2f} TB/s")
    with open(os.path.join(out, "glif_eval_timing.txt"), "w") as f:
        f.write("\n".join(tl) + "\n")
    print("\n".join(tl))


if __name__ == "__main__":
    main()
