"""The unfused eval plan of an MS SDformerFlow model: every neuron call of the reference's layer sequence is "fp32 pre-activation in
memory -> the general neuron launch (`hip.neuron_fwd`: csrc/neuron.hip) -> u8 spikes in the layout the next product reads".

The products, the BN / bias / residual / scatter epilogues, the row maps, the deconvolution routes and the recording route are
`MSFlowEngine`'s: this class only chooses its non-fused branches - no branch that asks the library whether it can fuse a neuron is
taken - and composes the attention and the MLP from `hip.spike_gemm` and the neuron launch.  Two users:

  * a GLIF model (engine_glif.GLIFFlowEngine, a thin subclass): no fused epilogue has a GLIF form, this is its eval forward;
  * a membrane monitor (monitor.MembraneMonitor) on a `lif` / `if` / `plif` / `SLTTlif` model (`model.unfused_engine()`): with the
    pre-activation of every call in memory, the membrane of every call is one kernel variant away - while such a monitor runs a
    forward, every neuron launch goes to `sdf_neuron_vseq_fwd` with a transient fp32 `v_seq` buffer that has the spike buffer's own
    addressing, and every record hands the monitor the membrane view that lies where the recorded spikes lie.

Since every call's spikes are in memory anyway, the parity tape and the firing-rate monitor read them where they lie; the plain
forward launches the same kernels (and is bit-equal to the taped one).  For non-GLIF neurons the token gate is `hip.qk_gate` on the u8
spikes; its own neuron call `attn.sn2_q` and the dead score `attn.attn_sn` are RECOMPUTED for a monitor through the general launch
(`MSFlowEngine._rec_gates`): the gate's record is a recomputation, not a read-out of the gate kernel.

Not built: replicas in one launch sequence (`forward_replicas` goes sample by sample), `log=True`.
"""
import torch

from . import hip
from .engine import MSFlowEngine, attention_score
from .STSwinNet_SNN.Spiking_swin_transformer3D import get_window_size


class UnfusedFlowEngine(MSFlowEngine):
    what = "the unfused plan"

    # ------------------------------------------------------------------ the neuron launch, and the membrane it can keep
    # Whether this forward keeps membranes: a membrane monitor (monitor.MembraneMonitor) sets it around its forward, with itself as
    # `self.monitor`.
    _membranes = False
    _vbufs = None

    def _neuron_fwd(self, x, out, *args, **kw):
        if not self._membranes:
            return hip.neuron_fwd(x, out, *args, **kw)
        # one fp32 buffer per spike STORAGE, addressed as the spikes are: launches that fill slices of one image (the decoder's
        # sources) share it, and a record finds its membrane view by the spikes' own offset, shape and strides (_membrane_of)
        store = out.untyped_storage()
        key, n = store.data_ptr(), store.nbytes() // out.element_size()
        buf = self._vbufs.get(key)
        if buf is None or buf.numel() != n:
            buf = self._vbufs[key] = torch.empty(n, dtype=torch.float32, device=out.device)
        return hip.neuron_fwd(x, out, *args, v_seq=buf[out.storage_offset():], **kw)

    def _membrane_of(self, spikes):
        """The fp32 membrane view of a recorded spike tensor or view, and its buffer forgotten (the monitor keeps or drops the view)."""
        buf = self._vbufs.pop(spikes.untyped_storage().data_ptr(), None)
        if buf is None:
            raise hip.SdfError("membrane monitor: a neuron call's spikes were recorded that the general neuron launch did not write "
                               "(a fused branch was taken on the unfused plan)")
        return buf.as_strided(tuple(spikes.shape), tuple(spikes.stride()), spikes.storage_offset())

    def _rec(self, name, spikes, layout, steps=None):
        if not self._membranes:
            return super()._rec(name, spikes, layout, steps)
        if self.tape is not None:
            self.tape.append((name, spikes.clone(), layout))
        v = self._membrane_of(spikes)
        self.monitor.record(name, v if steps is None else v.view(steps, -1, v.shape[-1]), layout)

    def _rec_monitor(self, name, spikes, layout):
        if not self._membranes:
            return super()._rec_monitor(name, spikes, layout)
        self.monitor.record(name, self._membrane_of(spikes), layout)

    # ------------------------------------------------------------------ the base class's fused branches, switched off
    def _head_fused(self, T, H, W, num_ch):
        return False

    @staticmethod
    def _pred_head_fused(*a):
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
        self._neuron_fwd(src, s.view(-1)[c0:], D, hw, take, pitch, hw * pitch, cp, hw * cp, sn, rep=(B, D * hw * pitch, D * hw * cp))

    def patch_merge(self, x, s, packed=None, spikes=None):
        """The merge as the reference lays it out, in every mode (plain, taped, monitored: one route): a membrane record is the
        reference's tensor at this call - the 2x2 concatenation with its zero rows - which only the gathered launch lays out (the
        digit-plane merge runs the neuron on x and concatenates by operand addressing)."""
        lin, sn = self.merges[s] if packed is None else packed
        self._check_cl(x)
        return self._patch_merge_gathered(x, lin, sn, f"sttmultires_unet.encoders.swin3d.layers.{s}.downsample.sn.spiking_neuron.")

    def _decoder_image(self, i, level, y, skip, preds, ready, carried):
        if not self._membranes or not level.same:
            return super()._decoder_image(i, level, y, skip, preds, ready, carried)
        # the base class records a copy of the image in the reference's channel order [prediction | y | skip]; the membrane image gets
        # the same re-ordering (the copy is what the monitor reads, and keeps if asked)
        mon, self.monitor = self.monitor, None
        tape, self.tape = self.tape, None
        try:
            s, order = super()._decoder_image(i, level, y, skip, preds, ready, carried)
        finally:
            self.monitor, self.tape = mon, tape
        C1, C2 = y.shape[-1], skip.shape[-1]
        npred = self.preds[i - 1].nout if i > 0 else 0
        name = f"sttmultires_unet.decoders.{i}.sn.spiking_neuron."
        if tape is not None:
            tape.append((name, torch.cat([s[..., C1 + C2:C1 + C2 + npred], s[..., :C1 + C2]], -1), "BDHWC->TBCHW"))
        v = self._membrane_of(s)
        mon.record(name, torch.cat([v[..., C1 + C2:C1 + C2 + npred], v[..., :C1 + C2]], -1), "BDHWC->TBCHW")
        return s, order

    # ------------------------------------------------------------------ block
    def _token_gate(self, blk, qk, xs, Tq, B_, N1, name):
        """E = k gated by SN2_q(head sums of q), over the slice spikes xs (T', rows, C) u8; a monitor gets the gate's two neuron calls."""
        hip.qk_gate(qk[0], qk[1], xs, Tq, B_ * N1, xs.shape[-1], blk.sn2_q)
        if self.monitor is not None:
            self._rec_gates(blk, qk[0], xs, Tq, B_, N1)

    def attention(self, x, blk, score_out=None, emit=None):
        """x (B,D,H,W,C) += SSA(x), in place (reference Spiking_swin_transformer3D.py:781-821, 661-717, :840): slice neuron through the
        window row map -> q product + BN -> neuron -> k product + BN -> neuron with the positional encoding added -> token gate ->
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
        self._neuron_fwd(x, xs, Tq, 1, n, 0, 0, 0, n, blk.sn_proj, rowmap=rowmap, rowlen=Cc)
        self._rec(name + "proj_sn.spiking_neuron.", xs, "flat")
        pre = torch.empty((M, Cc), dtype=torch.float32, device=dev)
        qk = torch.empty((2, Tq, rows, Cc), dtype=torch.uint8, device=dev)
        hip.spike_gemm(xs, blk.q.Wp, pre, M, Cc, Cc, alpha=blk.q.alpha, beta=blk.q.beta)
        self._neuron_fwd(pre, qk[0], Tq, 1, n, 0, n, 0, n, blk.sn_q)
        self._rec(name + "sn_q.spiking_neuron.", qk[0], "flat")
        hip.spike_gemm(xs, blk.k.Wp, pre, M, Cc, Cc, alpha=blk.k.alpha, beta=blk.k.beta)
        # (the positional table is consumed as flat (Tq, N1, C) memory: the reference's raw reshape, :678-679)
        self._neuron_fwd(pre, qk[1], Tq, 1, n, 0, n, 0, n, blk.sn_k, add=blk.pe, add_st=N1 * Cc, add_period=N1 * Cc)
        self._rec(name + "sn_k.spiking_neuron.", qk[1], "flat")
        self._token_gate(blk, qk, xs, Tq, B_, N1, name)                                     # (E overwrites the slice spikes)
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
            raise NotImplementedError(f"log=True is not built for {self.what}: the attention score is only computed for a monitor")
        if replicas:
            raise hip.ReplicaGeometryError(f"{self.what} has no replica launch sequence: the samples go one by one")
        self._vbufs = {}
        try:
            return super().forward(x)
        finally:
            self._vbufs = {}
