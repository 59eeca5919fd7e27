"""Spike-forced oracle replay of a GLIF model's eval forward (TEST INFRASTRUCTURE): tests/replay.py's statement with the
delta-consistency rule of the GLIF recurrence, which `oracle.delta_consistent` does not have.

The rule, per neuron call, from v = 0, s = 0: at step t form u_t with the oracle's own expression (`glif_multistep`) from v and the
spike FOLLOWED so far; the reference decision is u_t - th >= 0; where |u_t - th| <= delta the decision is ambiguous and the run
follows the other implementation's spike, elsewhere the threshold's; then v = u_t.  `unexplained` = elements where that run differs
from the other implementation's spikes: must be 0.  delta = DELTA_ULPS * 2^-23 * max(rms(pre-activation), th)."""
import torch

import replay
import test_replay_gpu as R
from oracle import sdformer_oracle as O
from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import GatedLIFNode

# delta in ulps of max(rms(x), th).  replay.py's 16 rests on a measured need of 2.1 ulps (8x headroom).  The GLIF leak L can lie nearer 1
# than LIF's 1/2, so a rounding difference of an earlier pre-activation is carried further: measured on the MI355X over the two
# configurations of tests/test_glif_eval_gpu.py the departures from the reference's spikes need at most MEASURED_ULPS (2.20 at B = 1 in
# preds.0.sn, 2.75 at B = 2 in layers.0.swin_blocks.0.mlp.sn1) - above 2, so the delta is the smallest power of two at or above
# 8 x 2.75 = 22.  At 32 ulps 645 of 131 M (B = 1) and 639 of 188 M (B = 2) decisions are ambiguous: 4.9e-6 and 3.4e-6, under the 2e-5 cap.
MEASURED_ULPS = 2.75
DELTA_ULPS = 32.0

LOGIT_RANGE = {"v_threshold": (-3.5, -2.0), "linear_decay": (-6.0, -4.0)}              # every other gate logit: (-1, 1)


def redraw_gate_logits(model, seed=5):
    """Every parameter of every GatedLIFNode, in named_parameters() order, from ONE generator: with the synthetic default (all logits
    -0.1) 23 of the 78 neuron calls of the 3-encoder model never fire; with this draw none is silent (rates 0.11 .. 1.0)."""
    nodes = {name for name, m in model.named_modules() if isinstance(m, GatedLIFNode)}
    g = torch.Generator().manual_seed(seed)
    n = 0
    with torch.no_grad():
        for name, p in model.named_parameters():
            owner, _, leaf = name.rpartition(".")
            if owner in nodes:
                lo, hi = LOGIT_RANGE.get(leaf, (-1.0, 1.0))
                p.copy_((torch.rand(p.shape, generator=g) * (hi - lo) + lo).to(p.device))
                n += 1
    assert n == 8 * len(nodes) and n > 0
    return model


def build(size):
    """The 3-encoder MS model of tests/test_replay_gpu.py with GLIF neurons and redrawn gate logits
    -> (model on the GPU in eval mode, oracle state dict, oracle config)."""
    model, _, ocfg = R.build("glif", size, en4=False)
    redraw_gate_logits(model)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}
    return model, sd, ocfg


def glif_delta_consistent(x, got, sd, prefix, delta):
    """-> dict(unexplained, flips, ambiguous, needed, n) as `oracle.delta_consistent` returns them, for the GLIF recurrence."""
    got = got.to(x.dtype)
    g = lambda k: torch.sigmoid(sd[prefix + k].float())
    al, be, ga = g("alpha"), g("beta"), g("gamma")
    leak, th = 1 - al * (1 - g("tau")), g("v_threshold")

    def step(t, v, spike):                                            # the oracle's expression (glif_multistep)
        inp = x[t] * (1 - be * (1 - torch.sigmoid(sd[prefix + "conduct"][t].float())))
        u = (leak * v - (1 - al) * g("linear_decay")) + inp
        return u - leak * v * ga * spike - (1 - ga) * g("v_subreset") * spike

    v, s = 0.0, torch.zeros_like(x[0])                                # the followed run
    vr, sr = 0.0, torch.zeros_like(x[0])                              # the plain reference run (for the flip count)
    unexplained = flips = ambiguous = 0
    needed = 0.0
    for t in range(x.shape[0]):
        u = step(t, v, s)
        margin = u - th
        dec = (margin >= 0).to(x.dtype)
        amb = margin.abs() <= delta
        s = torch.where(amb, got[t], dec)
        unexplained += int((s != got[t]).sum())
        ambiguous += int(amb.sum())
        used = amb & (got[t] != dec)
        if used.any():
            needed = max(needed, float(margin.abs()[used].max()))
        v = u
        ur = step(t, vr, sr)
        sr = (ur - th >= 0).to(x.dtype)
        flips += int((sr != got[t]).sum())
        vr = ur
    return {"unexplained": unexplained, "flips": flips, "ambiguous": ambiguous, "needed": needed, "n": got.numel()}


def run(engine, x_gpu, oracle_call, delta_ulps=DELTA_ULPS):
    """Taped forward of `engine` on x_gpu, then `oracle_call()` with every taped call's spikes forced and checked
    -> (gpu flows, replayed flows, per-call report, tape {name: (u8 spikes, layout)})."""
    engine.tape = []
    try:
        with torch.no_grad():
            flows = engine.forward(x_gpu)
        torch.cuda.synchronize()
        tape = {}
        for name, t, layout in engine.tape:
            assert name not in tape, f"neuron call recorded twice: {name}"
            tape[name] = (t, layout)
    finally:
        engine.tape = None
    report, used = [], set()

    def hook(prefix, x, s, ncfg, sd_):
        if prefix not in tape:
            report.append({"layer": prefix, "forced": False, "n": s.numel()})
            return s
        t, layout = tape[prefix]
        used.add(prefix)
        got = replay.to_reference_layout(t, layout, x.shape).cpu().to(x.dtype)
        th = float(torch.sigmoid(sd_[prefix + "v_threshold"].float()))
        scale = max(float(x.pow(2).mean().sqrt()), th)
        ulp = 2.0 ** -23 * scale
        r = glif_delta_consistent(x, got, sd_, prefix, delta_ulps * ulp)
        r.update(layer=prefix, forced=True, needed_ulps=r["needed"] / ulp, scale=scale, rate=float(got.mean()))
        report.append(r)
        return got

    O.NEURON_HOOK = hook
    try:
        with torch.no_grad():
            ref = oracle_call()
    finally:
        O.NEURON_HOOK = None
    missing = set(tape) - used
    assert not missing, f"taped calls the oracle never asked for: {sorted(missing)[:5]}"
    return flows, ref, report, tape
