#!/usr/bin/env python3
"""Generate tests/golden/flow_loss.npz from the REAL reference's loss class (loss/flow_supervised.py, loaded by file path: it imports
only torch, numpy and math; gamma=None) behind the models' own tail - sum over time, F.interpolate by the level's factor - on the CPU.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_flow_loss.py <path of the reference checkout>      (or SDF_REFERENCE=<path>)

Seeded raw predictions (T, B, 2, h, w) for the factors (4, 2, 1) below a 16 x 24 frame, B = 2, T = 3; a label that equals
pred.sum(0) * flow_scaling exactly at a few pixels of the last level; a 0 / 1 mask.  Stored: `pred0..2`, `label`, `mask`, `flow_scaling`,
`lambda_mod`, and the class's loss with autograd's gradients with respect to the raw predictions, once computed in fp32 (`loss32`,
`grad32_<i>`) and once in fp64 from the same fp32 inputs (`loss64`, `grad64_<i>`).  Only inputs and recorded results are stored."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
B, T, H, W = 2, 3, 16, 24
FACTORS = (4, 2, 1)
FLOW_SCALING, LAMBDA_MOD = 1.5, 0.75


def run(loss_fn, preds, label, mask, dtype):
    leaves = [p.detach().to(dtype).clone().requires_grad_(True) for p in preds]
    flows = []
    for p in leaves:
        f = p.sum(0)
        flows.append(F.interpolate(f, scale_factor=(H / f.shape[-2], W / f.shape[-1])))
    loss = loss_fn(flows, label.to(dtype), mask.to(dtype))
    loss.backward()
    return loss.detach().numpy(), [p.grad.numpy() for p in leaves]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("reference_flow_supervised", os.path.join(ref, "loss", "flow_supervised.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    config = {"metrics": {"flow_scaling": FLOW_SCALING}, "loss": {"lambda_mod": LAMBDA_MOD, "lambda_ang": 0.0}}
    loss_fn = mod.flow_loss_supervised(config, "cpu")
    g = torch.Generator().manual_seed(20240917)
    preds = [torch.randn((T, B, 2, H // s, W // s), generator=g) for s in FACTORS]
    label = torch.randn((B, 2, H, W), generator=g) * 2
    mask = (torch.rand((B, 1, H, W), generator=g) < 0.7).float()
    preds[-1][..., 3, 5:9] = torch.round(preds[-1][..., 3, 5:9] * 4) / 4        # quarters: their sum * 1.5 is exact in fp32 and fp64
    hit = preds[-1].sum(0) * FLOW_SCALING
    label[:, :, 3, 5:9] = hit[:, :, 3, 5:9]
    mask[:, :, 3, 5:9] = 1.0
    out = {"label": label.numpy(), "mask": mask.numpy(), "flow_scaling": np.float64(FLOW_SCALING), "lambda_mod": np.float64(LAMBDA_MOD)}
    for i, p in enumerate(preds):
        out[f"pred{i}"] = p.numpy()
    for name, dtype in (("32", torch.float32), ("64", torch.float64)):
        loss, grads = run(loss_fn, preds, label, mask, dtype)
        out["loss" + name] = loss
        for i, gr in enumerate(grads):
            out[f"grad{name}_{i}"] = gr
    np.savez(os.path.join(HERE, "flow_loss.npz"), **out)
    print("wrote flow_loss.npz: loss", float(out["loss32"]), float(out["loss64"]))


if __name__ == "__main__":
    main()
