#!/usr/bin/env python3
"""Generate tests/golden/glif_grads.npz, sltt_grads.npz and glif_train_block.npz from the REAL reference: autograd through the
reference's `Spiking_neuron(neuron_type="glif" | "SLTTlif", surrogate_fun="surrogate.ATan()")` in train mode, multi-step, and one
TRAIN-mode forward + backward of its MS swin block built with glif neurons.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_glif_train.py

Same conventions as make_golden.py / make_golden_plif_train.py (whose helpers and stubs it imports): seeded inputs, weights from
`sdformerflow_amd.synthetic`, DropPath replaced by the identity, a fixed random sample of the block's large tensors.

glif_grads.npz, per T in {2, 4, 10} and per-step size N in {256, 105 as (3, 7, 5), 3076}: the gate logits (drawn with the call
make_golden.gold_neurons_extra draws them with), the derived table [L, Dk, g, R, th, c_0 .. c_{T-1}] computed on the CPU in the
reference's op order, the spikes, dL/dx and the gradient of every logit.  The inputs are 3 * synth_uniform(seed) with two column
blocks overwritten: `tie` columns hold an x for which u - th == 0 exactly at t = 0 (found by the nextafter search of
make_golden_plif_train.tie_inputs, their number recorded; whether one exists depends on the parity of th + Dk on the grid of
x * c_0, so the logits are the first of up to 16 seeded draws for which one does), `hard` columns hold x = 2.5 at every step, so
spikes follow each other and the non-detached s_{t-1} path carries gradient.  Beside them, from an fp64 evaluation of the reference recurrence's BPTT on the fp32
trajectory: the 5 + T table gradients (`gtab64`) and the sum of the absolute values of their terms (`gtab_abs`), the scale the
fixed-order fp32 reduction of the kernel is held against.  The script asserts that this evaluation, chained to the logits, agrees
with the reference's autograd, and that oracle.sdformer_oracle.glif_multistep reproduces the reference's spikes in every decision.

sltt_grads.npz: the reference's SLTTLIFNode in train mode is driven step by step (it is a single-step node: `step_mode == 's'` is
asserted in its constructor) through the stubs' multi-step loop; the committed stubs run it, so its own autograd is what is stored."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stubs on sys.path)
from make_golden import functional, ref_ann, ref_swin, rnd  # noqa: E402
from make_golden_plif_train import sample  # noqa: E402
from oracle import sdformer_oracle as O  # noqa: E402

SHAPES = {"N256": (256,), "N105": (3, 7, 5), "N3076": (3076,)}
GATES = ("alpha", "beta", "gamma", "tau", "v_threshold", "linear_decay", "v_subreset", "conduct")
V_TH = 0.1


def cpu_table(sd):
    """[L, Dk, g, R, th, c_t] in fp32 on the CPU, the products in the reference's order (Spiking_submodules.py:153-162)."""
    s = {k: torch.sigmoid(sd["spiking_neuron." + k].float()) for k in GATES}
    head = torch.stack([1 - s["alpha"] * (1 - s["tau"]), (1 - s["alpha"]) * s["linear_decay"], s["gamma"],
                        (1 - s["gamma"]) * s["v_subreset"], s["v_threshold"]])
    return torch.cat([head, 1 - s["beta"] * (1 - s["conduct"])])


def glif_tie_inputs(tab):
    """fp32 x whose first-step membrane (0 - Dk) + x * c_0 equals th exactly (the reference's op order from v = 0, s = 0)."""
    Dk, th, c0 = tab[1], tab[4], tab[5]
    found = []
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        xv = np.float32((float(th) + float(Dk)) / float(c0))
        for _ in range(64):
            u = (torch.tensor(0.0) - Dk) + torch.tensor(xv) * c0
            if float(u - th) == 0.0 and float(xv) not in found:
                found.append(float(xv))
            xv = np.nextafter(xv, direction)
    return found


def bptt64(x, tab, g, alpha=2.0):
    """The reference recurrence's BPTT in fp64 on the fp32 trajectory (u_t, s_t from the fp32 forward): (grad_tab, sum |terms|)."""
    T = x.shape[0]
    L, Dk, gg, R, th = (tab[i] for i in range(5))
    v, s, us, ss = torch.zeros_like(x[0]), torch.zeros_like(x[0]), [], []
    for t in range(T):                                              # fp32 forward, the reference's order
        lv = L * v
        u = (lv - Dk) + x[t] * tab[5 + t]
        u = u - lv * gg * s - R * s
        s = (u - th >= 0).float()
        v = u
        us.append(u)
        ss.append(s)
    d = lambda a: a.double()
    L, Dk, gg, R, th = d(L), d(Dk), d(gg), d(R), d(th)
    gt, ga = torch.zeros(5 + T, dtype=torch.float64), torch.zeros(5 + T, dtype=torch.float64)
    gu = torch.zeros_like(d(x[0]))
    for t in range(T - 1, -1, -1):
        u, s = d(us[t]), d(ss[t])
        S = d(g[t]) + gu * (-(L * u) * gg - R)
        V = gu * (L - L * gg * s)
        sg = alpha / 2 / (1 + (np.pi / 2 * alpha * (u - th)) ** 2) * S
        gu = V + sg
        vp, sp = (d(us[t - 1]), d(ss[t - 1])) if t > 0 else (torch.zeros_like(u), torch.zeros_like(u))
        terms = {0: gu * (vp - vp * gg * sp), 1: -gu, 2: -gu * L * vp * sp, 3: -gu * sp, 4: -sg, 5 + t: gu * d(x[t])}
        for i, term in terms.items():
            gt[i] += term.sum()
            ga[i] += term.abs().sum()
    return gt, ga


def gold_glif_grads():
    from models.STSwinNet_SNN.Spiking_modules import Spiking_neuron
    out = {}
    with torch.enable_grad():
        for T in (2, 4, 10):
            n = Spiking_neuron(num_steps=T, neuron_type="glif", surrogate_fun="surrogate.ATan()")
            for draw in range(16):                                    # the first draw of logits for which an exact tie exists in fp32
                sd = {k: rnd(tuple(v.shape), 900 + 1000 * draw + 16 * T + i, -1.0, 2.0)
                      for i, (k, v) in enumerate(n.state_dict().items())}
                tab = cpu_table(sd)
                ties = glif_tie_inputs(tab)
                if ties:
                    break
            assert ties, "no fp32 input puts u - th at exactly 0"
            n.load_state_dict(sd)
            n.train()
            for k, v in sd.items():
                out[f"T{T}/{k}"] = v
            out[f"T{T}_tab"], out[f"T{T}_ties"], out[f"T{T}_tie_x"] = tab, np.array(len(ties)), np.array(ties[0], dtype=np.float32)
            for si, (tag, shape) in enumerate(SHAPES.items()):
                N = int(np.prod(shape))
                blk = 64 if N >= 256 else 8
                x0 = (3.0 * rnd((T,) + shape, 1000 + 10 * T + si, -0.3, 0.6)).reshape(T, N)
                x0[0, :blk] = ties[0]                                # u - th == 0 exactly at t = 0: `>= 0` must fire
                x0[:, blk:2 * blk] = 2.5                             # consecutive spikes
                x0 = x0.reshape((T,) + shape)
                g = rnd((T,) + shape, 1100 + 10 * T + si, -1.0, 2.0)
                functional.reset_net(n)
                n.zero_grad()
                x = x0.clone().requires_grad_(True)
                s = n(x)
                s.backward(g.reshape(s.shape))
                s = s.detach().reshape(x0.shape)
                key = f"T{T}_{tag}"
                assert bool((s.reshape(T, N)[0, :blk] == 1).all()), "the tie columns did not fire at t = 0"
                hard = s.reshape(T, N)[:, blk:2 * blk]
                assert bool((hard[:-1] * hard[1:]).sum() > 0), "no consecutive spikes in the hard-driven block"
                want = O.glif_multistep(x0, sd, "spiking_neuron.")
                assert int((want != s).sum()) == 0, "the oracle's restatement differs from the reference on these inputs"
                out[f"{key}_s"], out[f"{key}_gx"] = s.to(torch.uint8), x.grad.clone()
                for k in GATES:
                    out[f"{key}_g/{k}"] = getattr(n.spiking_neuron, k).grad.clone()
                gt, ga = bptt64(x0.reshape(T, N), tab, g.reshape(T, N))
                out[f"{key}_gtab64"], out[f"{key}_gtab_abs"] = gt, ga
                # the fp64 evaluation, chained to the logits through the table expression, is the reference's autograd
                logits = {k: sd["spiking_neuron." + k].double().requires_grad_(True) for k in GATES}
                sg = {k: torch.sigmoid(v) for k, v in logits.items()}
                tab64 = torch.cat([torch.stack([1 - sg["alpha"] * (1 - sg["tau"]), (1 - sg["alpha"]) * sg["linear_decay"], sg["gamma"],
                                                (1 - sg["gamma"]) * sg["v_subreset"], sg["v_threshold"]]),
                                   1 - sg["beta"] * (1 - sg["conduct"])])
                (tab64 * gt).sum().backward()
                for k in GATES:
                    ref = out[f"{key}_g/{k}"].double()
                    assert (logits[k].grad - ref).abs().max() <= 1e-4 * ga.max(), (key, k, logits[k].grad, ref)
                print(f"{key}: rate {float(s.mean()):.3f}  ties {len(ties)}")
    mg.save("glif_grads", **out)


def gold_sltt_grads():
    from models.STSwinNet_SNN.Spiking_modules import Spiking_neuron
    from make_golden_plif_train import tie_inputs
    out = {"v_th": np.array(V_TH)}
    N = 256
    with torch.enable_grad():
        for T in (2, 4, 10):
            base = rnd((T, N), 1200 + T, -0.3, 0.6)
            g = rnd((T, N), 1300 + T, -1.0, 2.0)
            for tag, vr in (("soft", None), ("hard", 0.0), ("hard005", 0.05)):
                ties = tie_inputs(0.5, 0.0 if vr is None else vr, vr)     # tau = 2: the multiplier 0.5 (division by 2 is exact)
                x0 = base.clone()
                x0[:, :64] = 0.1
                if ties:
                    x0[0, 64:128] = ties[0]
                out[f"{tag}_T{T}_ties"] = np.array(len(ties))
                out[f"{tag}_T{T}_tie_x"] = np.array(ties[0] if ties else 0.0, dtype=np.float32)
                for detach in (True, False):
                    n = Spiking_neuron(num_steps=T, neuron_type="SLTTlif", v_th=V_TH, v_reset=vr, surrogate_fun="surrogate.ATan()",
                                       tau=2.0, detach_reset=detach)
                    functional.set_step_mode(n, "m")
                    functional.reset_net(n)
                    n.train()
                    x = x0.clone().requires_grad_(True)
                    s = n(x)
                    s.backward(g)
                    key = f"{tag}_{'detach' if detach else 'nodetach'}_T{T}"
                    out[f"{key}_s"], out[f"{key}_gx"] = s.detach().to(torch.uint8), x.grad.clone()
                assert torch.equal(out[f"{tag}_detach_T{T}_gx"], out[f"{tag}_nodetach_T{T}_gx"])
    mg.save("sltt_grads", **out)


def gold_glif_train_block():
    """Train-mode MS swin block with glif neurons: the shape and seeds of make_golden_plif_train.gold_plif_train_block."""
    out = {}
    C, nH, (B, H, W), shift = 96, 3, (2, 18, 21), (1, 4, 4)
    with torch.enable_grad():
        blk = ref_swin.MS_Spiking_SwinTransformerBlock3D(C, (H, W), nH, window_size=(2, 9, 9), shift_size=shift, norm_layer="BN",
                                                         **mg.spk_kwargs("glif", 4))
        mg.load_synth(blk)
        with torch.no_grad():
            for i, (n, prm) in enumerate(blk.named_parameters()):
                if ".spiking_neuron." in n:                           # gate logits drawn as above, a function of the position only
                    prm.copy_(rnd(tuple(prm.shape), 1400 + i, -1.0, 2.0))
                    out[f"w/{n}"] = prm.detach().clone()
        blk.train()
        mg._no_drop_path(blk)
        functional.reset_net(blk)
        x = rnd((B, 4, H, W, C), 17, -0.5, 1.0).requires_grad_(True)
        g = rnd((B, 4, H, W, C), 18, -1.0, 2.0)
        Hp, Wp = -(-H // 9) * 9, -(-W // 9) * 9
        wsz, ssz = ref_ann.get_window_size((4, H, W), (2, 9, 9), shift)
        mask = ref_swin.compute_mask(4, Hp, Wp, wsz, ssz, torch.device("cpu"))
        y = blk(x, mask)
        y.backward(g)
        sample(out, "y", y)
        sample(out, "gx", x.grad)
        out["cfg"] = np.array([B, H, W, *shift])
        for n, prm in blk.named_parameters():
            if prm.grad is not None:
                sample(out, f"g/{n}", prm.grad, 2048)
        for n, buf in blk.named_buffers():
            if n.endswith(("running_mean", "running_var")):
                out[f"r/{n}"] = buf.clone()
    mg.save("glif_train_block", **out)


if __name__ == "__main__":
    gold_glif_grads()
    gold_sltt_grads()
    gold_glif_train_block()
