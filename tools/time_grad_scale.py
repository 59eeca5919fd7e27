"""The tail of the configs[3] training step under a loss scaler, on the en4 model's parameters with the gradients of one real backward
(multiplied by the scale): the figures of DESIGN.md section 7 / profiles/grad_scale_timing.txt.

  (a) train.BucketAdamW.step(100.0, scaler=LossScaler): statistics, coefficient + scaler, scaled update on csrc/grad_step.hip
  (b) train.BucketAdamW.step(100.0): the tail without a scaler, measured in the same run
  (c) torch.amp.GradScaler + clip_grad_norm_ + torch.optim.AdamW (its default: foreach on the GPU): scaler.step, scaler.update
  (d) one micro-step of an accumulation: statistics, coefficient, hip.grad_scale in place on every bucket

Every variant is called round-robin, `--iters` times after `--warmup`, each call between two stream events AND inside a host clock that
ends in a device synchronise; the gradients are restored from a copy between calls, outside the timed window.  Event span = device
time from the call's first to its last operation, including gaps the host leaves between launches; wall = host clock to the
synchronise; host = the host clock around the call alone, before the synchronise - what the call costs the Python thread.  If the
deferred read of the skip verdict waited for the device, (a)'s host time would be its wall time.  Medians over the calls.

usage: python tools/time_grad_scale.py [--iters 50] [--warmup 5] [--out FILE]    (one MI355X)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from sdformerflow_amd import train  # noqa: E402
from sdformerflow_amd.harness import prepare_chunk  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_voxel  # noqa: E402

SCALE = 1024.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X (no CPU timing)"
    dev = torch.device("cuda:0")
    model, _ = bench.build_model("lif", dev)
    chunk = prepare_chunk(synth_voxel(1, 10, 288, 384, seed=1238)).to(dev)
    label, mask = (t.to(dev) for t in synth_label(1, 288, 384, seed=4321))
    buckets = train.GradientBuckets(model.parameters())
    train.train_step(model, torch.optim.SGD(model.parameters(), lr=0.0), chunk, label, mask, buckets=buckets, clip_grad=None)   # one real backward
    saved = [f.clone() for f in buckets.flat]
    scaled = [f * SCALE for f in saved]
    live = [p for p in model.parameters() if p.grad is not None]
    n_live = sum(p.numel() for p in live)
    norm = float(torch.linalg.vector_norm(torch.cat([f.double() for f in saved])))

    opt = train.BucketAdamW(buckets, lr=1e-4, weight_decay=0.01)
    scaler = train.LossScaler(init_scale=SCALE, device=dev)
    topt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    ts = torch.amp.GradScaler("cuda", init_scale=SCALE)
    ts.scale(torch.zeros((), device=dev))
    st = opt.stats

    def restore(src):
        for f, s in zip(buckets.flat, src):
            f.copy_(s)
        st.valid = st.clipped = False

    def tail_torch():
        torch.nn.utils.clip_grad_norm_(live, 100.0)
        ts.step(topt)
        ts.update()

    def micro_step():
        st.compute()
        st.clip(100.0)
        st.scale_inplace()

    variants = [("(a) BucketAdamW.step(100.0, scaler=LossScaler)", scaled, lambda: opt.step(100.0, scaler=scaler)),
                ("(b) BucketAdamW.step(100.0)", saved, lambda: opt.step(100.0)),
                ("(c) GradScaler + clip_grad_norm_ + AdamW", scaled, tail_torch),
                ("(d) accumulation micro-step: clip in place", saved, micro_step)]
    span = {name: [] for name, _, _ in variants}
    wall = {name: [] for name, _, _ in variants}
    host = {name: [] for name, _, _ in variants}
    for it in range(args.warmup + args.iters):
        for name, src, fn in variants:
            restore(src)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= args.warmup:
                span[name].append(e0.elapsed_time(e1))
                host[name].append((t1 - t0) * 1e3)
                wall[name].append((t2 - t0) * 1e3)
    lines = [f"en4 (lif) at 288 x 384: {len(buckets.params)} parameters in {len(buckets.flat)} buckets, {n_live} floats with a gradient; gradient norm "
             f"{norm:.4g} times the loss scale {SCALE:g}, clip 100 (on the scaled norm); {args.iters} calls each after {args.warmup} warm-up, "
             f"round-robin; median [min .. max] in ms",
             f"{'':50s} {'event span':>28s} {'wall to synchronise':>28s} {'host time of the call':>28s}"]
    for name, _, _ in variants:
        s, w, h = span[name], wall[name], host[name]
        lines.append(f"{name:50s} {statistics.median(s):8.3f} [{min(s):7.3f} .. {max(s):7.3f}] {statistics.median(w):8.3f} [{min(w):7.3f} .. {max(w):7.3f}] "
                     f"{statistics.median(h):8.3f} [{min(h):7.3f} .. {max(h):7.3f}]")
    a, b = span[variants[0][0]], span[variants[1][0]]
    lines.append(f"(a) - (b), medians of the event span: {statistics.median(a) - statistics.median(b):+.3f} ms; the spread of (b) in this run "
                 f"(max - min): {max(b) - min(b):.3f} ms")
    lines.append(f"steps skipped by the scaler in this run: {scaler.skipped}; scale afterwards {scaler.get_scale():g} (torch's {ts.get_scale():g})")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
