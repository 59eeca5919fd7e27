"""Eval-mode HIP plan of an MS SDformerFlow model built with GLIF neurons (`neuron_type: glif`, the reference's GatedLIFNode).

No fused epilogue has a GLIF form, so the model runs on the unfused plan (engine_unfused.UnfusedFlowEngine): every neuron call of the
reference's layer sequence is "fp32 pre-activation in memory -> `hip.glif_neuron_fwd` (csrc/neuron.hip glif_neuron_kernel: the general
launch's addressing, BN affine, positional add, row-map gather and channel-slice output; `hip.neuron_fwd` sends a GlifParams there) ->
u8 spikes in the layout the next product reads".  What is GLIF's own is here: how a node is packed, and the token gate
`hip.qk_gate_glif` (csrc/qk_gate.hip), whose own output is what the tape and the firing-rate monitor record for `attn.sn2_q`.

Gate tables: each node's [L, Dk, g, R, th, c_0 .. c_{T-1}] is formed ONCE at pack time on the host - fp32 sigmoids of the CPU, the
products in the reference's order - and uploaded, as `bn_affine` forms eval-BN: given equal pre-activations the spikes are then
the CPU reference's bit for bit.  (`GatedLIFNode.table()`, with the device's sigmoids, stays what training and the module-level call
use.)

Not built: fused epilogues, replicas in one launch sequence (`forward_replicas` goes sample by sample), `log=True`, membranes (a
GatedLIFNode keeps no `v_seq` in the reference either).
"""
import torch

from . import hip
from .engine import _np, attention_score
from .engine_unfused import UnfusedFlowEngine

_GATES = ("alpha", "beta", "gamma", "tau", "v_threshold", "linear_decay", "v_subreset", "conduct")


def gate_table(node):
    """[L, Dk, g, R, th, c_0 .. c_{T-1}] of a GatedLIFNode from a HOST copy of its 7 + T logits (reference Spiking_submodules.py:153-162)."""
    s = {k: torch.sigmoid(getattr(node, k).detach().float().cpu()) for k in _GATES}
    head = torch.stack([1 - s["alpha"] * (1 - s["tau"]), (1 - s["alpha"]) * s["linear_decay"], s["gamma"],
                        (1 - s["gamma"]) * s["v_subreset"], s["v_threshold"]])
    return torch.cat([head, 1 - s["beta"] * (1 - s["conduct"])]).contiguous()


def _glif_np(sn_module, device):
    n = sn_module.spiking_neuron
    if n.kind != "glif":
        return _np(sn_module, device)
    return hip.GlifParams(gate_table(n).to(device))


class GLIFFlowEngine(UnfusedFlowEngine):
    _np = staticmethod(_glif_np)
    what = "a GLIF model"

    def _token_gate(self, blk, qk, xs, Tq, B_, N1, name):
        rows, Cc = B_ * N1, xs.shape[-1]
        gate = torch.empty((Tq, rows, blk.nH), dtype=torch.uint8, device=xs.device) if self.taped else None
        hip.qk_gate_glif(qk[0], qk[1], xs, Tq, rows, Cc, blk.sn2_q.tab, gate=gate)
        if gate is not None:
            self._rec(name + "sn2_q.spiking_neuron.", gate, "flat")
        if self.monitor is not None:           # the dead attention score (:709-711) is a neuron call the monitor counts
            s = attention_score(xs, blk.attn_sn, blk.nH, Tq, B_, N1)
            self.monitor.record(name + "attn_sn.spiking_neuron.", s.to(torch.uint8), "flat")
