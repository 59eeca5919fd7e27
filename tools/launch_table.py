#!/usr/bin/env python3
"""Per-launch table of ONE forward from the library's own launch log (hip.launch_log: HIP events around every kernel launch, no
profiler): duration, workgroups, chip time = min(workgroups / resident slots, 1) x duration, per launch and summed per kernel.
usage: launch_table.py [lif|psn|planes3|config4|sew] [R = 1] [seq] [launches]
    lif / psn: the headline configuration; planes3: lif on three bf16 weight planes (no digit planes); config4: T = 20, 480 x 640, batch 4;
    sew: the SEW model (3 encoders)          R > 1: forward_replicas over R samples          seq: also the sequence
    launches: ONLY the sequence, without timings - kernel name with its template arguments, workgroups, threads, dynamic LDS bytes
    per line, repeated blocks folded: two builds that issue the same launches print the same text"""
import os, re, sys, torch, yaml
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from sdformerflow_amd import hip
from sdformerflow_amd.harness import prepare_chunk
from sdformerflow_amd.synthetic import synth_state_dict, synth_voxel
kind = sys.argv[1] if len(sys.argv) > 1 else "lif"
R = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dev = torch.device("cuda:0")
if kind in ("config4", "sew"):
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4, SpikingformerFlowNet
    T, H, W, B = (20, 480, 640, 4) if kind == "config4" else (10, 288, 384, 1)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif", num_steps=T)
    cfg["model"].update(num_bins=T)
    cfg["swin_transformer"].update(input_size=[H, W])
    if kind == "sew":
        cfg["swin_transformer"].update(swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    model = (SpikingformerFlowNet if kind == "sew" else MS_SpikingformerFlowNet_en4)(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model = model.eval().to(dev)
    x = prepare_chunk(synth_voxel(B * R, T, H, W, seed=1239)).to(dev)
else:
    model, _ = bench.build_model("lif" if kind == "planes3" else kind, dev)
    if kind == "planes3":
        model.gemm_nsplit = 3
    x = torch.cat([bench.synthetic_chunk(1235 + i) for i in range(R)], 0).to(dev)
fwd = (lambda: model.forward_replicas(x)) if R > 1 else (lambda: model(x))
with torch.no_grad():
    for _ in range(3):
        fwd()
    torch.cuda.synchronize()
    with hip.launch_log() as log:
        fwd()


def short(name, width=70):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\b(sdfmm|sdf)::", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"\(.*$", "", name)[:width]                # (the parameter list goes, the template arguments stay)


if "launches" in sys.argv:
    print(f"# {kind}, {R} sample(s) per launch sequence: {len(log.rows)} launches (workgroups threads LDS-bytes kernel)")
    lines, i = [f"{wgs} {thr} {lds} {short(k, None)}" for k, wgs, thr, lds, _ in log.rows], 0

    def repeats(i, p):                              # how many times in a row the p lines from i on stand there
        c = 1
        while lines[i + c * p:i + (c + 1) * p] == lines[i:i + p]:
            c += 1
        return c
    while i < len(lines):                           # (a block of launches repeated back to back - the blocks of a stage - is printed once)
        p, c = next(((p, repeats(i, p)) for p in range(1, 40) if repeats(i, p) > 1), (1, 1))
        print("\n".join(lines[i:i + p]) if c == 1 else f"{c} times {{\n  " + "\n  ".join(lines[i:i + p]) + "\n}")
        i += p * c
    sys.exit(0)


def chip_us(wgs, us):
    return min(wgs / 256.0, 1.0) * us               # (one workgroup per compute unit as the unit: an upper bound where several fit a CU)


tot = sum(r[4] for r in log.rows)
chip = sum(chip_us(r[1], r[4]) for r in log.rows)
print(f"# {kind}, {R} sample(s) per launch sequence: {len(log.rows)} launches, {tot:.1f} us of kernel time = {tot / R:.1f} us per sample; "
      f"chip time {chip:.1f} us = {chip / R:.1f} us per sample")
if "seq" in sys.argv:
    for i, (k, wgs, thr, lds, us) in enumerate(log.rows):
        print(f"{i:4d} {us:8.1f} us {wgs:6d} wg x {thr:4d} thr {lds:6d} B lds  chip {chip_us(wgs, us):7.1f}  {short(k)}")
agg = {}
for k, wgs, thr, lds, us in log.rows:
    a = agg.setdefault(short(k), [0, 0.0, 0.0, 0])
    a[0] += 1; a[1] += us; a[2] += chip_us(wgs, us); a[3] = max(a[3], wgs)
print(f"{'kernel':72s} {'n':>4s} {'us':>9s} {'us/sample':>10s} {'chip us':>9s} {'max wgs':>8s}")
for k, (n, us, ch, mw) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    print(f"{k:72s} {n:4d} {us:9.1f} {us / R:10.1f} {ch:9.1f} {mw:8d}")
