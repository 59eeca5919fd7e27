"""The tail of the configs[3] training step - what runs behind loss.backward() - five ways, on the en4 model's parameters with the
gradients of one real backward: the figures of DESIGN.md section 7 / profiles/grad_step_timing.txt.

  (a) torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (its default: foreach on the GPU)        - what train_step ran before
  (b) the same with AdamW(fused=True)
  (c) train.BucketAdamW.step(100.0): statistics, clip coefficient and update on csrc/grad_step.hip
  (d) (c) + train.get_grads: the `vis.store_grads` record by one read-back
  (e) the reference's get_grads on the clipped gradients: three .item() per weight (the record alone, no optimiser)

Every variant is called round-robin, `--iters` times after `--warmup`, each call between two stream events AND inside a host clock that
ends in a device synchronise; the gradients are restored from a copy between calls, outside the timed window (clip_grad_norm_ scales
them in place).  Event span = device time from the call's first to its last operation, including gaps the host leaves between
launches; wall = host clock to the synchronise.  Medians over the calls; (d) and (e) end in a read-back by themselves.

usage: python tools/time_grad_step.py [--iters 50] [--warmup 5] [--out FILE]    (one MI355X)"""
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


def reference_get_grads(named_parameters):
    """What the reference's loop records per step (restated: |grad| mean, min, max of every weight, one .item() each)."""
    record = {}
    for n, p in named_parameters:
        if p.requires_grad and "weight" in n and p.grad is not None:
            a = p.grad.abs()
            record[f"{n}_mean"], record[f"{n}_min"], record[f"{n}_max"] = a.mean().item(), a.min().item(), a.max().item()
    return record


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
    live = [p for p in model.parameters() if p.grad is not None]
    n_live, n_all = sum(p.numel() for p in live), sum(p.numel() for p in buckets.params)
    norm = float(torch.linalg.vector_norm(torch.cat([f.double() for f in saved])))

    opt_a = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    opt_b = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01, fused=True)
    opt_c = train.BucketAdamW(buckets, lr=1e-4, weight_decay=0.01)

    def restore():
        for f, s in zip(buckets.flat, saved):
            f.copy_(s)
        buckets.stats.valid = buckets.stats.clipped = False

    def tail_torch(opt):
        torch.nn.utils.clip_grad_norm_(live, 100.0)
        opt.step()

    def tail_d():
        opt_c.step(100.0)
        return train.get_grads(model, buckets)

    variants = [("(a) clip_grad_norm_ + AdamW (default)", lambda: tail_torch(opt_a)),
                ("(b) clip_grad_norm_ + AdamW(fused=True)", lambda: tail_torch(opt_b)),
                ("(c) BucketAdamW.step(100.0)", lambda: opt_c.step(100.0)),
                ("(d) (c) + get_grads read-back", tail_d),
                ("(e) reference get_grads, 3 .item() per weight", lambda: reference_get_grads(model.named_parameters()))]
    span = {name: [] for name, _ in variants}
    wall = {name: [] for name, _ in variants}
    for it in range(args.warmup + args.iters):
        for name, fn in variants:
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= args.warmup:
                span[name].append(e0.elapsed_time(e1))
                wall[name].append((t1 - t0) * 1e3)
    n_rec = len(reference_get_grads(model.named_parameters()))
    lines = [f"en4 (lif) at 288 x 384: {len(buckets.params)} parameters, {n_all} floats in {len(buckets.flat)} buckets, {n_live} of them with a gradient; "
             f"gradient norm {norm:.4g}, clip 100; {args.iters} calls each after {args.warmup} warm-up, round-robin; median [min .. max] in ms",
             f"{'':50s} {'event span':>28s} {'wall to synchronise':>28s}"]
    for name, _ in variants:
        s, w = span[name], wall[name]
        lines.append(f"{name:50s} {statistics.median(s):8.3f} [{min(s):7.3f} .. {max(s):7.3f}] {statistics.median(w):8.3f} [{min(w):7.3f} .. {max(w):7.3f}]")
    c = statistics.median(span["(c) BucketAdamW.step(100.0)"])
    lines.append(f"(c) moves 32 bytes per float with a gradient (4 read by the statistics; 16 read and 12 written by the update): "
                 f"{32 * n_live / 1e6:.1f} MB, {32 * n_live / c / 1e6:.0f} GB/s over the event span (launch gaps included: not a kernel rate)")
    lines.append(f"the store_grads record holds {n_rec} values")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
