#!/usr/bin/env python3
"""The rendering kernels' cost on one MI355X - the figures of DESIGN.md section 7 / profiles/flow_render_timing.txt.

1  One 288 x 384 sample rendered four ways (flow, gtflow, events, submission): the device time of the library's launches
   (hip.launch_log) and of the whole sequence with torch.quantile between the event stages (HIP events), against the wall time of the
   numpy / matplotlib-order restatement (tests/vis_cases.py) of the same sample on the host, the fp32 copies it needs included.
2  harness.evaluate_stream with and without renders_out (all four buffers), same process, alternating legs, median of the rounds.

    python tools/flow_render_measure.py --out profiles/flow_render_timing.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=10)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X (no CPU fallback)"
    import yaml
    import vis_cases as V
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4
    from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type="lif")
    cfg["swin_transformer"]["input_size"] = [288, 384]
    model = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model = model.eval().to(dev)
    cfg["loader"] = dict(cfg["loader"], crop=[288, 384], polarity=True)
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    cfg["vis"] = dict(cfg.get("vis") or {}, store=False)
    distinct = []
    for i in range(min(args.distinct, args.samples)):
        label, mask = synth_label(1, 480, 640, seed=4321 + i)
        distinct.append((synth_voxel(1, 10, 480, 640, seed=1235 + i).to(dev), mask[:, 0].to(dev), label.to(dev)))
    samples = [distinct[i % len(distinct)] for i in range(args.samples)]
    say(f"flow_render_measure: {torch.cuda.get_device_name(0)}; en4 lif, 10 bins, 480 x 640 -> 288 x 384")

    # 1 - one sample
    vox, _, label = distinct[0]
    crop = (288, 384)
    lab = harness.center_crop(label, crop).contiguous()
    with torch.no_grad():
        flow = model(hip.prepare_chunk(vox, crop))["flow"][-1].contiguous()
    bufs = {k: torch.empty((1,) + crop + (3,), dtype=torch.uint8, device=dev) for k in ("flow", "gtflow", "events")}
    sub = torch.empty((1,) + crop + (3,), dtype=torch.uint16, device=dev)

    def render():
        hip.flow_image(flow, out=bufs["flow"])
        hip.flow_image(lab, out=bufs["gtflow"])
        hip.event_image(vox, crop=crop, out=bufs["events"])
        hip.flow_submission(flow, out=sub)
    for _ in range(5):
        render()
    torch.cuda.synchronize()
    per = {}
    reps = 20
    for _ in range(reps):
        with hip.launch_log() as log:
            render()
        for name, wgs, thr, lds, us in log.rows:
            key = name.split("flow_render_")[-1].split("(")[0]
            per.setdefault(key, []).append(us)
    n_launch = len(log.rows)
    med = {k: statistics.median(v) * (len(v) // reps) for k, v in per.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        render()
    e1.record()
    torch.cuda.synchronize()
    seq_us = e0.elapsed_time(e1) / 50 * 1e3

    def host():
        f, g, v = flow[0].cpu().numpy(), lab[0].cpu().numpy(), harness.center_crop(vox, crop)[0].cpu().numpy()
        return V.flow_image_ref(f), V.flow_image_ref(g), V.event_image_ref(V.event_counts_ref(v)), V.submission_ref(f)
    host()
    t = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        t.append(time.perf_counter() - t0)
    say(f"one 288 x 384 sample, flow + gtflow + events + submission: {n_launch} library launches, "
        f"{sum(med.values()):.1f} us of device time in them (launch log, medians of {reps}): " +
        ", ".join(f"{k} {v:.1f}" for k, v in med.items()))
    say(f"  the whole sequence on the stream, torch.quantile between the event stages included: {seq_us:.1f} us per sample (HIP events, 50 runs)")
    say(f"  the numpy restatement of the same sample on the host, its three fp32 copies included: {statistics.median(t) * 1e3:.1f} ms wall "
        f"(median of 5) = x{statistics.median(t) * 1e6 / seq_us:.0f} the stream's sequence")

    # 2 - the streamed evaluation with and without the render buffers
    n = args.samples
    renders = {k: torch.empty((n,) + crop + (3,), dtype=torch.uint8, device=dev) for k in ("flow", "gtflow", "events")}
    renders["submission"] = torch.empty((n,) + crop + (3,), dtype=torch.uint16, device=dev)
    ev = harness.StreamEvaluator(model, cfg, dev, replicas=args.replicas, streams=args.streams)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    leg(lambda: ev.run(samples))                                        # (captures the graphs)
    leg(lambda: ev.run(samples, renders_out=renders))
    ta, tb = [], []
    for r in range(args.rounds):
        a, res_a = leg(lambda: ev.run(samples))
        b, res_b = leg(lambda: ev.run(samples, renders_out=renders))
        ta.append(a)
        tb.append(b)
        say(f"  round {r}: evaluate_stream {n / a:8.1f} samples/s   with renders_out (4 buffers) {n / b:8.1f} samples/s")
    ma, mb = statistics.median(ta), statistics.median(tb)
    say(f"median: evaluate_stream {n / ma:.1f} samples/s, with renders_out {n / mb:.1f} samples/s: x{ma / mb:.3f} "
        f"(+{(mb - ma) * 1e6 / n:.1f} us per sample); metrics equal: {res_a == res_b}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
