"""Eval-mode HIP plan of an MS SDformerFlow model built with GLIF neurons (`neuron_type: glif`, the reference's GatedLIFNode).

No fused epilogue has a GLIF form, so every neuron call of the reference's layer sequence is "fp32 pre-activation in memory ->
`hip.glif_neuron_fwd` (csrc/neuron.hip glif_neuron_kernel: the general launch's addressing, BN affine, positional add, row-map gather
and channel-slice output) -> u8 spikes in the layout the next product reads", and the token gate is `hip.qk_gate_glif`
(csrc/qk_gate.hip).  The products, the BN / bias / residual / scatter epilogues, the row maps, the deconvolution routes and the
recording route are `MSFlowEngine`'s: this class only chooses its non-fused branches and composes the attention and the MLP from
`hip.spike_gemm` and the neuron launch.  Since every call's spikes are in memory anyway, the parity tape and the firing-rate monitor
read them where they lie; the plain forward launches the same kernels (and is bit-equal to the taped one).

Gate tables: each node's [L, Dk, g, R, th, c_0 .. c_{T-1}] is formed ONCE at pack time on the host - fp32 sigmoids of the CPU, the
products in the reference's order - and uploaded, as `bn_affine` forms eval-BN: given equal pre-activations the spikes are then
the CPU reference's bit for bit.  (`GatedLIFNode.table()`, with the device's sigmoids, stays what training and the module-level call
use.)

Not built: fused epilogues, replicas in one launch sequence (`forward_replicas` goes sample by sample), `log=True`.
"""
import torch

from . import hip
from .engine import MSFlowEngine, _np, attention_score
from .STSwinNet_SNN.Spiking_swin_transformer3D import get_window_size

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


class GLIFFlowEngine(MSFlowEngine):
    _np = staticmethod(_glif_np)

    # ------------------------------------------------------------------ the base class's fused branches, switched off
    def _head_fused(self, T, H, W, num_ch):
        return False

    def _conv3x3(self, s, Wp, Cout, stride=1, bn=None, resid=None, sn=None, membrane=False):
        """The fp32 form of the convolution (BN, + resid), then the neuron launch where the caller hands a neuron over."""
        m = super()._conv3x3(s, Wp, Cout, stride=stride, bn=bn, resid=resid if sn is None or membrane else None)
        if sn is None:
            return m
        sp = self._neuron_bd(m, sn)
        return (m, sp) if membrane else sp

    def _next_spikes(self, x, blk, sn):
        return None

    def _prepare_decoder_images(self, feats, y0, out_size, levels):
        return None

    def _slice_neuron(self, src, take, pitch, s, c0, sn):
        """One launch for the whole batch: the samples are the descriptor's outermost dimension."""
        B, D, h, w, cp = s.shape
        hw = h * w
        hip.glif_neuron_fwd(src, s.view(-1)[c0:], D, hw, take, pitch, hw * pitch, cp, hw * cp, sn.tab,
                            rep=(B, D * hw * pitch, D * hw * cp))

    # ------------------------------------------------------------------ block
    def attention(self, x, blk, score_out=None, emit=None):
        """x (B,D,H,W,C) += SSA(x), in place (reference Spiking_swin_transformer3D.py:781-821, 661-717, :840): slice neuron through the
        window row map -> q product + BN -> neuron -> k product + BN -> neuron with the positional encoding added -> GLIF token gate ->
        projection through the head scramble with bias + BN + scatter + residual."""
        self._check_cl(x)
        B, D, H, W, Cc = x.shape
        ws, ss = get_window_size((D, H, W), blk.window_size, blk.shift_size)
        if tuple(ws) != tuple(blk.window_size):
            raise hip.SdfError(f"feature map {(D, H, W)} is smaller than the window {tuple(blk.window_size)}: the positional encoding of "
                               "Spiking_QK_WindowAttention3D is defined for the nominal window only (reference Spiking_swin_transformer3D.py:678)")
        rowmap, B_ = self._slice_map(B, D, H, W, ws, ss)
        Tq, N1 = ws[0], ws[1] * ws[2]
        rows = B_ * N1
        M, n = Tq * rows, rows * Cc
        dev, name = x.device, blk.name + "attn."
        xs = torch.empty((Tq, rows, Cc), dtype=torch.uint8, device=dev)
        hip.neuron_fwd(x, xs, Tq, 1, n, 0, 0, 0, n, blk.sn_proj, rowmap=rowmap, rowlen=Cc)
        self._rec(name + "proj_sn.spiking_neuron.", xs, "flat")
        pre = torch.empty((M, Cc), dtype=torch.float32, device=dev)
        qk = torch.empty((2, Tq, rows, Cc), dtype=torch.uint8, device=dev)
        hip.spike_gemm(xs, blk.q.Wp, pre, M, Cc, Cc, alpha=blk.q.alpha, beta=blk.q.beta)
        hip.neuron_fwd(pre, qk[0], Tq, 1, n, 0, n, 0, n, blk.sn_q)
        self._rec(name + "sn_q.spiking_neuron.", qk[0], "flat")
        hip.spike_gemm(xs, blk.k.Wp, pre, M, Cc, Cc, alpha=blk.k.alpha, beta=blk.k.beta)
        # (the positional table is consumed as flat (Tq, N1, C) memory: the reference's raw reshape, :678-679)
        hip.neuron_fwd(pre, qk[1], Tq, 1, n, 0, n, 0, n, blk.sn_k, add=blk.pe, add_st=N1 * Cc, add_period=N1 * Cc)
        self._rec(name + "sn_k.spiking_neuron.", qk[1], "flat")
        gate = torch.empty((Tq, rows, blk.nH), dtype=torch.uint8, device=dev) if self.taped else None
        hip.qk_gate_glif(qk[0], qk[1], xs, Tq, rows, Cc, blk.sn2_q.tab, gate=gate)          # (E overwrites the slice spikes)
        if gate is not None:
            self._rec(name + "sn2_q.spiking_neuron.", gate, "flat")
        if self.monitor is not None:           # the dead attention score (:709-711) is a neuron call the monitor counts
            s = attention_score(xs, blk.attn_sn, blk.nH, Tq, B_, N1)
            self.monitor.record(name + "attn_sn.spiking_neuron.", s.to(torch.uint8), "flat")
        hip.spike_gemm(xs, blk.p.Wp, x, M, Cc, Cc, bias=blk.p.bias, alpha=blk.p.alpha, beta=blk.p.beta, resid=x, out_rowmap=rowmap,
                       zg=(blk.nH, Tq, B_, N1))
        self._emitted = False
        return x

    def mlp(self, x, blk, ws=None, s1_ready=False, emit_next=None):
        """x (B,D,H,W,C) += MLP(x) over the true time axis D, in place (reference :164-181, :845)."""
        self._check_cl(x)
        B, D, H, W, Cc = x.shape
        tok, Ch = B * D * H * W, blk.fc1.N
        s1 = self._neuron_bd(x, blk.sn1)
        self._rec(blk.name + "mlp.sn1.spiking_neuron.", s1, "BDHWC->TBHWC")
        h = torch.empty((B, D, H, W, Ch), dtype=torch.float32, device=x.device)
        hip.spike_gemm(s1, blk.fc1.Wp, h, tok, Ch, Cc, alpha=blk.fc1.alpha, beta=blk.fc1.beta)
        s2 = self._neuron_bd(h, blk.sn2)
        self._rec(blk.name + "mlp.sn2.spiking_neuron.", s2, "BDHWC->TBHWC")
        hip.spike_gemm(s2, blk.fc2.Wp, x, tok, Cc, Ch, alpha=blk.fc2.alpha, beta=blk.fc2.beta, resid=x)
        return x

    def swin_block(self, x, s, i, emit_next=None):
        blk = self.stages[s][i]
        return self.mlp(self.attention(x, blk), blk)

    def forward(self, x, scores=None, replicas=False):
        if scores is not None:
            raise NotImplementedError("log=True is not built for a GLIF model: the attention score is only computed for the firing-rate monitor")
        if replicas:
            raise hip.ReplicaGeometryError("a GLIF model has no replica launch sequence: the samples go one by one")
        return super().forward(x)
