#!/usr/bin/env python3
"""Generate tests/golden/sew_train_block.npz and sew_train_step_forced.npz from the REAL reference: TRAIN-mode forward + backward of
its SEW swin block (Spiking_SwinTransformerBlock3D, C = 96, nH = 3, window (2, 9, 9), shifted and unshifted, lif and psn) and of the
3-encoder SpikingformerFlowNet at 144 x 192, batch 2, with the oracle's spike-forced replay of the latter.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_sew_train.py

Same conventions as make_golden.py (whose helpers and stubs it imports, and which it leaves unchanged): seeded inputs, weights from
`sdformerflow_amd.synthetic`, DropPath replaced by the identity; only the reference's OUTPUTS are stored - of the block's large
tensors a fixed random sample of elements (positions stored beside them), to keep the files small."""
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stubs on sys.path)
from make_golden import functional, ref_ann, ref_swin, rnd  # noqa: E402
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

SAMPLE = 2048                      # elements kept of a large tensor
BLOCKS = (("lif_w", "lif", (1, 4, 18, 21), (0, 0, 0)), ("lif_sw", "lif", (1, 4, 18, 21), (1, 4, 4)),
          ("psn_w", "psn", (1, 4, 9, 21), (0, 0, 0)), ("psn_sw", "psn", (1, 4, 18, 21), (1, 4, 4)))
STEP = (2, 144, 192, 1234 + 9)     # batch, H, W, voxel seed (label: synth_label's default seed)


def sample(out, key, t, n=SAMPLE):
    """t itself when it has at most n elements; else n elements at seeded random flat positions (`key@idx` int32, `key` the values)."""
    t = t.detach().reshape(-1)
    if t.numel() <= n:
        out[key] = t.clone()
        return
    idx = np.sort(np.random.default_rng(zlib.crc32(key.encode())).choice(t.numel(), n, replace=False)).astype(np.int32)
    out[key + "@idx"], out[key] = idx, t[torch.from_numpy(idx).long()].clone()


def gold_sew_train_block():
    out = {}
    C, nH = 96, 3
    with torch.enable_grad():
        for tag, kind, (B, D, H, W), shift in BLOCKS:
            blk = ref_swin.Spiking_SwinTransformerBlock3D(C, (H, W), nH, window_size=(2, 9, 9), shift_size=shift, norm_layer="BN",
                                                          qk_scale=0.125, **mg.spk_kwargs(kind, D))
            mg.load_synth(blk)
            blk.train()
            mg._no_drop_path(blk)
            functional.reset_net(blk)
            x = rnd((B, D, H, W, C), 21, -0.5, 1.5).requires_grad_(True)
            g = rnd((B, D, H, W, C), 22, -1.0, 2.0)
            Hp, Wp = -(-H // 9) * 9, -(-W // 9) * 9
            wsz, ssz = ref_ann.get_window_size((D, H, W), (2, 9, 9), shift)
            mask = ref_swin.compute_mask(D, Hp, Wp, wsz, ssz, torch.device("cpu"))
            y = blk(x, mask)
            y.backward(g)
            out[f"{tag}_cfg"] = np.array([B, D, H, W, *shift])
            out[f"{tag}_scale"] = np.array(float(blk.attn.scale))
            sample(out, f"{tag}_y", y)
            sample(out, f"{tag}_gx", x.grad)
            for n, prm in blk.named_parameters():
                if prm.grad is not None:
                    sample(out, f"{tag}_g/{n}", prm.grad)
            for n, buf in blk.named_buffers():
                if n.endswith(("running_mean", "running_var")):
                    sample(out, f"{tag}_r/{n}", buf)
    mg.save("sew_train_block", **out)


def step_chunk():
    B, H, W, seed = STEP
    vox = synth_voxel(B, 10, H, W, seed=seed)
    chunk = torch.cat((torch.relu(vox).unsqueeze(2), torch.relu(-vox).unsqueeze(2)), dim=2)
    lo, hi = chunk[chunk != 0].min(), chunk[chunk != 0].max()
    chunk[chunk != 0] = (chunk[chunk != 0] - lo) / (hi - lo)
    label, mask = synth_label(B, H, W)
    return chunk, label, mask


def gold_sew_train_step_forced():
    """`make_golden.gold_train_step_forced` for the SEW model: the reference's train-mode step with every neuron layer's spikes
    taped, then the oracle's TRAIN-mode `forward_sew_flownet` with those spikes forced.  Stored: the loss pair, per parameter the
    reference's gradient norm and max|g_oracle - g_reference| / max|g_reference|, per forced layer (flips, unexplained, decisions)."""
    from models.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    from loss.flow_supervised import flow_loss_supervised
    from oracle import sdformer_oracle as O
    B, H, W, _ = STEP
    out = {"cfg": np.array(STEP)}
    for kind in ("lif", "psn"):
        config = mg.en4_config(kind)
        config["swin_transformer"].update(input_size=[H, W], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
        chunk, label, mask = step_chunk()
        with torch.enable_grad():
            model = SpikingformerFlowNet(config["model"].copy(), config["swin_transformer"].copy())
            mg.load_synth(model)
            model.train()
            mg._no_drop_path(model)
            functional.reset_net(model)
            tape = {}
            hooks = [m.register_forward_hook(lambda mod, inp, o, n=n: tape.__setitem__(n + ".", o.detach().clone()))
                     for n, m in model.named_modules() if n.endswith(".spiking_neuron")]
            res = model(chunk)
            loss = flow_loss_supervised(config, "cpu")(res["flow"], label, mask, gamma=None)
            loss.backward()
            for h in hooks:
                h.remove()
            ref_grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in model.named_parameters()}
            shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()
                      if not k.endswith(("num_batches_tracked", "relative_position_index", "relative_coords_table"))}
        sd = synth_state_dict(shapes, 0, -0.1)                  # the weights and running statistics BEFORE the step
        sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and not k.endswith(("running_mean", "running_var")) else v.clone())
              for k, v in sd.items()}
        ocfg = {"neuron": O.NeuronCfg(kind, 0.1, None, 2.0, 10), "num_bins": 10, "window_size": (2, 9, 9), "depths": [2, 2, 6],
                "num_heads": [3, 6, 12]}
        report = []

        def force(prefix, x, sd=sd, ocfg=ocfg):
            got = tape.get(prefix)
            if got is None:
                return None
            xd = x.detach()
            delta = 16 * 2.0 ** -23 * max(float(xd.pow(2).mean().sqrt()), 0.1)
            r = O.delta_consistent(xd, got.reshape(xd.shape), ocfg["neuron"], {k: v.detach() for k, v in sd.items()}, prefix, delta)
            report.append((prefix, r["flips"], r["unexplained"], r["n"]))
            return got.reshape(x.shape)

        O.TRAIN, O.NEURON_FORCE = O.TrainCtx(), force
        try:
            with torch.enable_grad():
                flows = O.forward_sew_flownet(chunk, sd, ocfg)
                oloss = O.flow_loss_supervised(flows, label, mask, 1.0, 1.0)
                oloss.backward()
        finally:
            O.TRAIN, O.NEURON_FORCE = None, None
        names, norms, rel = [], [], []
        for n, g in ref_grads.items():
            og = sd[n].grad
            names.append(n)
            if g is None or float(g.abs().max()) == 0.0:
                assert og is None or float(og.abs().max()) == 0.0, n
                norms.append(-1.0)
                rel.append(-1.0)
                continue
            norms.append(float(g.double().norm()))
            if n.endswith("attn.proj.bias"):
                # a bias in front of a batch-statistics BatchNorm: its true gradient is zero, both sides hold rounding noise
                rel.append(float((og - g).abs().max() / ref_grads[n[:-4] + "weight"].abs().max()))
            else:
                rel.append(float((og - g).abs().max() / g.abs().max()))
        worst = max(rel)
        print(f"  sew_train_step_forced[{kind}]: loss reference {float(loss):.8f} oracle {float(oloss):.8f}; {len(report)} layers forced, "
              f"{sum(r[1] for r in report)} decisions differ, {sum(r[2] for r in report)} unexplained of {sum(r[3] for r in report)}; "
              f"worst parameter-gradient deviation {worst:.2e} ({names[int(np.argmax(rel))]})")
        out[f"{kind}_loss"] = np.array([float(loss), float(oloss)])
        out[f"{kind}_grad_names"] = np.array(names)
        out[f"{kind}_grad_norms"], out[f"{kind}_grad_rel"] = np.array(norms, dtype=np.float64), np.array(rel, dtype=np.float64)
        out[f"{kind}_layers"] = np.array([r[0] for r in report])
        out[f"{kind}_flips_unexplained_n"] = np.array([[r[1], r[2], r[3]] for r in report], dtype=np.int64)
    mg.save("sew_train_step_forced", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["block", "step"]
    if "block" in which:
        gold_sew_train_block()
    if "step" in which:
        gold_sew_train_step_forced()
