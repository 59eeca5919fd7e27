#!/usr/bin/env python3
"""Generate tests/golden/ann_train_step.npz from the REAL reference: one TRAIN-mode forward + backward of the ANN STTFlowNet
(configs/train_DSEC_supervised_STT_voxel.yml at 144 x 192, batch 2, 20 bins: stage maps 36x48, 18x24, 9x12, so padding tokens
and shifted windows are both present) with the reference's loss (`flow_loss_supervised`, gamma None).

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_ann_train.py

Same conventions as make_golden.py (whose helpers it imports): weights regenerated from `sdformerflow_amd.synthetic`, DropPath
replaced by the identity so that the fixture is a function of the seeded inputs only; only the reference's OUTPUTS are stored."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stubs on sys.path)
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_voxel  # noqa: E402

SKIP = ("relative_position_index", "relative_coords_table", "num_batches_tracked")
B, BINS, H, W, SEED = 2, 20, 144, 192, 2026

# full gradient tensors kept beside the per-parameter norms
FULL = ["sttmultires_unet.encoders.swin3d.layers.0.swin_blocks.1.attn.qkv.bias",            # stage 0: padded and shifted
        "sttmultires_unet.encoders.swin3d.layers.2.swin_blocks.0.norm1.weight",
        "sttmultires_unet.preds.2.conv2d.weight", "sttmultires_unet.preds.2.conv2d.bias"]
FULL += [f"sttmultires_unet.encoders.swin3d.layers.{i}.swin_blocks.1.attn.cpb_mlp.{p}" for i in range(3)
         for p in ("0.weight", "0.bias", "2.weight")]
BN = "sttmultires_unet.encoders.swin3d.patch_embed.residual_encoding.resblock1.bn1"


def gold_ann_train_step():
    from models.STSwinNet.STSwinNet import STTFlowNet
    from loss.flow_supervised import flow_loss_supervised
    cfg = mg.YAMLParser("/root/reference/configs/train_DSEC_supervised_STT_voxel.yml")
    config = cfg.combine_entries(cfg.config)
    config["swin_transformer"]["input_size"] = [H, W]
    out = {}
    with torch.enable_grad():
        model = STTFlowNet(config["model"].copy(), config["swin_transformer"].copy())
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.endswith(SKIP)}
        model.load_state_dict(synth_state_dict(shapes), strict=False)
        model.train()
        mg._no_drop_path(model)
        vox = synth_voxel(B, BINS, H, W, seed=SEED)
        label, mask = synth_label(B, H, W, seed=SEED + 1)
        res = model(vox, None)
        lf = flow_loss_supervised(config, "cpu")
        loss = lf(res["flow"], label, mask, gamma=None)
        loss.backward()
        out["cfg"] = np.array([B, BINS, H, W, SEED])
        out["flow_scaling"], out["lambda_mod"] = np.array(float(lf.flow_scaling)), np.array(float(lf.lambda_mod))
        out["loss"] = np.array(float(loss))
        for i, f in enumerate(res["flow"]):
            out[f"flow{i}_abs_mean"] = np.array(float(f.abs().mean()))
        names, norms = [], []
        params = dict(model.named_parameters())
        for n, prm in params.items():
            names.append(n)
            norms.append(float(prm.grad.double().norm()) if prm.grad is not None else -1.0)
            if n.endswith("logit_scale"):
                out["g/" + n] = prm.grad.clone()
        out["grad_names"], out["grad_norms"] = np.array(names), np.array(norms, dtype=np.float64)
        for n in FULL:
            out["g/" + n] = params[n].grad.clone()
        bufs = dict(model.named_buffers())
        for s in ("running_mean", "running_var"):
            out[f"r/{BN}.{s}"] = bufs[f"{BN}.{s}"].clone()
    mg.save("ann_train_step", **out)


if __name__ == "__main__":
    gold_ann_train_step()
