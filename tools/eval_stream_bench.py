#!/usr/bin/env python3
"""harness.evaluate against harness.evaluate_stream on one MI355X, same process, alternating legs, median of the rounds.

Workload: the en4 LIF model at 288 x 384 (bench.py's), device-resident preprocessed synthetic samples (synthetic.synth_voxel /
synth_label, 10 bins, 480 x 640, centre-cropped by the loop), batch 1.  Also, with HIP events: the AEE + AAE classes against
hip.flow_metrics on one flow map, harness.prepare_chunk(center_crop(.)) against hip.prepare_chunk on one voxel; and the launch log
(sdf_launch_log) of one eagerly issued group of `--replicas` samples.  `--headline` = bench.py's `value` from a run on the same box:
the streamed rate is reported as a fraction of it.

    python tools/eval_stream_bench.py --out profiles/eval_stream_bench.txt [--headline 854.0]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=40, help="distinct synthetic voxels / labels; the samples cycle through them")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replicas", type=int, default=10)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--headline", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X (no CPU fallback)"
    import yaml
    from sdformerflow_amd import harness, hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4
    from sdformerflow_amd.loss.flow_supervised import AAE, AEE
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
    distinct = []
    for i in range(min(args.distinct, args.samples)):
        label, mask = synth_label(1, 480, 640, seed=4321 + i)
        distinct.append((synth_voxel(1, 10, 480, 640, seed=1235 + i).to(dev), mask[:, 0].to(dev), label.to(dev)))
    samples = [distinct[i % len(distinct)] for i in range(args.samples)]
    say(f"eval_stream_bench: {torch.cuda.get_device_name(0)}; en4 lif, 10 bins, 480 x 640 -> 288 x 384; {args.samples} device-resident samples "
        f"({len(distinct)} distinct, cycled); replicas {args.replicas}, streams {args.streams}; {args.rounds} rounds, legs alternating")

    ev = harness.StreamEvaluator(model, cfg, dev, replicas=args.replicas, streams=args.streams)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()                                                      # (both end in a device synchronise / a read-back)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res
    t_cold, res_s = leg(lambda: ev.run(samples))                        # (captures the graphs)
    _, res_e = leg(lambda: harness.evaluate(model, samples[:20], cfg, device=dev))
    te, ts = [], []
    for r in range(args.rounds):
        a, res_e = leg(lambda: harness.evaluate(model, samples, cfg, device=dev))
        b, res_s = leg(lambda: ev.run(samples))
        te.append(a)
        ts.append(b)
        say(f"  round {r}: evaluate {args.samples / a:8.1f} samples/s ({a * 1e3 / args.samples:.3f} ms/sample)   "
            f"evaluate_stream {args.samples / b:8.1f} samples/s ({b * 1e3 / args.samples:.3f} ms/sample)")
    me, ms = statistics.median(te), statistics.median(ts)
    say(f"median: evaluate {args.samples / me:.1f} samples/s, evaluate_stream {args.samples / ms:.1f} samples/s: x{me / ms:.2f}   "
        f"(first streamed run, graph capture included: {t_cold:.2f} s)")
    say(f"results: evaluate {res_e}")
    say(f"         evaluate_stream {res_s}")
    if args.headline:
        say(f"bench.py value on this box: {args.headline:.1f} samples/s -> evaluate_stream reaches {args.samples / ms / args.headline:.3f} of it")

    # the two ends of the loop on their own, HIP events on the launch stream
    vox, mask, label = distinct[0]
    lab, msk = harness.center_crop(label, (288, 384)).contiguous(), harness.center_crop(mask, (288, 384)).contiguous()
    with torch.no_grad():
        flow = model(hip.prepare_chunk(vox, (288, 384)))["flow"][-1]
    m4 = msk.unsqueeze(1)
    t_cls = event_ms(lambda: (AEE(flow, lab, m4, 1)(), AAE(flow, lab, m4, 1)()), 50)
    t_aee = event_ms(lambda: AEE(flow, lab, m4, 1)(), 50)
    table = torch.zeros((16, 8), dtype=torch.float64, device=dev)
    t_hip = event_ms(lambda: hip.flow_metrics(flow, lab, msk, None, 1, table=table), 200)
    flowR, labR, mskR = (t.repeat(args.replicas, *([1] * (t.dim() - 1))) for t in (flow, lab, msk))
    t_hipR = event_ms(lambda: hip.flow_metrics(flowR, labR, mskR, None, 1, table=table), 200)
    say(f"metrics, one 288 x 384 sample: AEE + AAE classes {t_cls * 1e3:.1f} us (AEE alone {t_aee * 1e3:.1f} us, no read-back counted); "
        f"hip.flow_metrics {t_hip * 1e3:.1f} us; a group of {args.replicas}: {t_hipR * 1e3:.1f} us = {t_hipR * 1e3 / args.replicas:.1f} us / sample")
    t_tprep = event_ms(lambda: harness.prepare_chunk(harness.center_crop(vox, (288, 384)), "minmax", None, True), 50)
    out = torch.empty((1, 10, 2, 288, 384), device=dev)
    t_hprep = event_ms(lambda: hip.prepare_chunk(vox, (288, 384), "minmax", None, out=out), 200)
    say(f"input preparation, one sample: harness.prepare_chunk(center_crop(.)) {t_tprep * 1e3:.1f} us (with its host round trips); "
        f"hip.prepare_chunk {t_hprep * 1e3:.1f} us")

    # where a group's time goes: the launch log of one eagerly issued group on one stream
    one = harness.StreamEvaluator(model, cfg, dev, replicas=args.replicas, streams=1, graphs=False)
    one.run(samples[:args.replicas])
    with hip.launch_log() as log:
        one.run(samples[:args.replicas])
    fam = {"prepare_chunk": 0.0, "flow_metrics": 0.0, "forward": 0.0}
    cnt = dict.fromkeys(fam, 0)
    for name, wgs, thr, lds, us in log.rows:
        k = "prepare_chunk" if "prepare_" in name else "flow_metrics" if "flow_metrics" in name else "forward"
        fam[k] += us
        cnt[k] += 1
    tot = sum(fam.values())
    say(f"launch log of one eager group of {args.replicas} (event-timed launches, one stream): " +
        "; ".join(f"{k}: {cnt[k]} launches, {fam[k]:.0f} us ({100 * fam[k] / tot:.1f} %)" for k in fam) +
        f"; sum {tot / 1e3:.2f} ms = {tot / 1e3 / args.replicas:.3f} ms / sample")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
