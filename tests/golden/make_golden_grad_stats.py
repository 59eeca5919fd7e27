#!/usr/bin/env python3
"""Generate tests/golden/grad_stats.npz from the REAL reference's get_grads (utils/gradients.py, loaded by file path: it imports only
torch) on a small seeded module, on the CPU.

Run in the build container only (needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_golden_grad_stats.py <path of the reference checkout>      (or SDF_REFERENCE=<path>)

The module: two convolutions, a BatchNorm and a Linear layer, one backward of a sum of squares - so that the record covers 4-D, 2-D
and 1-D weights, skips every bias, and one gradient (the BatchNorm weight's) is scaled down to denormals.  Stored: `names` (every
parameter, in named_parameters order), `grad/<name>` (fp32), `keys` / `values` (the record get_grads returned, float64), and the
same record once more after torch.nn.utils.clip_grad_norm_(parameters, 0.5) as `clip_keys` / `clip_values` with `clip_total` - the
order in which the training loop calls the two.  Only gradients and recorded values are stored."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SDF_REFERENCE")
    if not ref:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location("reference_gradients", os.path.join(ref, "utils", "gradients.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(20240611)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3, padding=1), torch.nn.BatchNorm2d(5), torch.nn.ReLU(), torch.nn.Conv2d(5, 2, 1),
                              torch.nn.Flatten(), torch.nn.Linear(2 * 7 * 9, 11))
    net(torch.randn(4, 3, 7, 9)).pow(2).sum().backward()
    with torch.no_grad():
        net[1].weight.grad.mul_(1e-42)                           # denormals
    out = {"names": np.array([n for n, _ in net.named_parameters()])}
    for n, p in net.named_parameters():
        out["grad/" + n] = p.grad.detach().numpy().copy()
    rec = mod.get_grads(net.named_parameters())
    out["keys"], out["values"] = np.array(list(rec)), np.array(list(rec.values()), dtype=np.float64)
    total = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
    rec = mod.get_grads(net.named_parameters())
    out["clip_keys"], out["clip_values"] = np.array(list(rec)), np.array(list(rec.values()), dtype=np.float64)
    out["clip_total"] = np.float64(total.item())
    np.savez(os.path.join(HERE, "grad_stats.npz"), **out)
    print("wrote grad_stats.npz:", len(out["keys"]), "recorded values, total norm", float(out["clip_total"]))


if __name__ == "__main__":
    main()
