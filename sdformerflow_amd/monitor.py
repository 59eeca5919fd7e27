"""Firing rates of every neuron call of a spiking model's HIP forward: the reference's `vis.monitor_fr`
(eval_DSEC_flow_SNN.py:22-24, 140-143, 223-227).

The reference puts an output monitor on every neuron module; each call records `cal_firing_rate(s_seq) = s_seq.flatten(1).mean(1)`,
one rate per time step, the mean of the per-layer means is printed and the records go to `firing_rate.csv`.  Here:

    mon = FiringRateMonitor(model)        # the MS (3 / 4 encoders) and SEW spiking models
    with mon:                             # or mon.enable() / mon.disable()
        model(x)                          # any number of forwards; each adds one record set
    mon.names                             # the neuron calls in the reference's call order (state_dict prefixes, no trailing dot)
    mon.counts()                          # (forwards, calls, Tmax) int64 on the device: spikes per call and time step
    mon.elements                          # per call: elements per time step
    mon.records                           # per forward, per call: a (T,) fp32 rate tensor (what fr_monitor.records holds)
    mon.mean()                            # what the reference prints
    mon.to_csv(path)

While enabled, the model's forward takes the engine's recording route - the kernels that leave every neuron layer's spikes in memory,
bit-equal to the plain forward - and every record enqueues one spike-count launch (hip.spike_count) on the tensor where it lies: no
copy is kept and the host does not synchronise per forward.  The denominator is the element count of the reference's own tensor at that
call, the zero rows it concatenates itself (odd sizes in front of a patch merging, padded window rows) included.  The two calls of
the MS attention whose spikes no kernel stores - the token gate `attn.sn2_q` and the dead score `attn.attn_sn` - are recomputed from
the recorded q spikes and the gated spikes (engine.MSFlowEngine._rec_gates): the gate's record is a recomputation, not a read-out of
the fused kernel.  (A GLIF model runs on the unfused plan, engine_glif.py: there the gate's record IS the gate kernel's own output.)
Eval mode, eager, one forward at a time: training mode, `forward_replicas` and graph capture are refused.
"""
import csv

import torch

from . import hip

_SUFFIX = ".spiking_neuron"


def neuron_call_names(model):
    """The neuron calls of one forward in the reference's call order (reference Spiking_modules.py:1770-1790, Spiking_swin_transformer3D.py
    :661-717 / :300-370, :164-181, Spiking_STSwinNet.py:161-182): 105 for the shipped 4-encoder MS model, 75 for the SEW model."""
    from .STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    sew = isinstance(model, SpikingformerFlowNet)
    unet = model.sttmultires_unet
    U = "sttmultires_unet."
    sw, pe = unet.encoders.swin3d, U + "encoders.swin3d.patch_embed."
    names = [pe + "head.sn"]
    for i in range(len(sw.patch_embed.residual_encoding.resblocks)):
        names += [pe + f"residual_encoding.resblocks.{i}.sn1", pe + f"residual_encoding.resblocks.{i}.sn2"]
    names.append(pe + "proj.sn")
    block = (("attn.sn_q", "attn.sn_k", "attn.sn_v", "attn.proj_sn", "mlp.sn1", "mlp.sn2") if sew else
             ("attn.proj_sn", "attn.sn_q", "attn.sn_k", "attn.sn2_q", "attn.attn_sn", "mlp.sn1", "mlp.sn2"))
    for li, layer in enumerate(sw.layers):
        for bi in range(len(layer.swin_blocks)):
            names += [U + f"encoders.swin3d.layers.{li}.swin_blocks.{bi}.{n}" for n in block]
        if layer.downsample is not None:
            names.append(U + f"encoders.swin3d.layers.{li}.downsample.sn")
    for i in range(len(unet.resblocks)):
        names += [U + f"resblocks.{i}.sn1", U + f"resblocks.{i}.sn2"]
    for i in range(len(unet.decoders)):
        names.append(U + f"decoders.{i}.sn")
        if not sew:                                      # (the SEW predictions are plain convolutions)
            names.append(U + f"preds.{i}.sn")
    return [n + _SUFFIX for n in names]


class FiringRateMonitor:
    """Per-step spike counts of every neuron call of `model`'s eval forwards while enabled (see the module's text).  `forwards`: rows
    the count table starts with; it doubles when they run out."""

    def __init__(self, model, forwards=16):
        from .STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
        if not isinstance(model, MS_SpikingformerFlowNet):
            raise hip.SdfError(f"FiringRateMonitor counts spikes: {type(model).__name__} is not a spiking model of this package (the ANN "
                               "model has no neuron calls); use MS_SpikingformerFlowNet(_en4) or SpikingformerFlowNet")
        self.model = model
        self.names = neuron_call_names(model)
        self._index = {n: i for i, n in enumerate(self.names)}
        unet = model.sttmultires_unet
        self.Tmax = max(int(unet.steps), int(unet.window_size[0]))
        if self.Tmax > 64:
            raise hip.SdfError(f"FiringRateMonitor: {self.Tmax} time steps; the count kernel takes at most 64")
        self._reserve = max(int(forwards), 1)
        self.reset()

    # ------------------------------------------------------------------ switching
    def enable(self):
        other = getattr(self.model, "_fr_monitor", None)
        if other is not None and other is not self:
            raise RuntimeError("another FiringRateMonitor is enabled on this model: disable() it first")
        self.model._fr_monitor = self
        return self

    def disable(self):
        if getattr(self.model, "_fr_monitor", None) is self:
            self.model._fr_monitor = None
        return self

    @property
    def enabled(self):
        return getattr(self.model, "_fr_monitor", None) is self

    def __enter__(self):
        return self.enable()

    def __exit__(self, *exc):
        self.disable()

    def reset(self):
        """Forget every record (the table is allocated again at the next forward)."""
        self._table, self._n = None, 0
        self._steps, self._elements = [], []             # per forward: T and elements per step of every call
        self._seen = None

    # ------------------------------------------------------------------ the forward (called by the model)
    def forward(self, x, scores=None):
        """One monitored forward of the model's packed plan (whichever rebuild of it): engine.forward on the recording route with every
        record counted into this forward's rows of the table.  The refusals come first: the plan is not even packed (its weight
        kernels and host copies) for a forward that is refused."""
        if not x.is_cuda:
            raise hip.SdfError("input must be a GPU tensor (no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a firing-rate monitor is enabled during graph capture: its forward takes the eager recording route and "
                               "grows a table - disable() the monitor around the capture, or run the monitored forwards eagerly")
        engine = self.model.eval_engine()
        self._room(x.device)
        self._seen = [None] * len(self.names)
        engine.monitor = self
        try:
            flows = engine.forward(x, scores)
            missing = [n for n, s in zip(self.names, self._seen) if s is None]
            if missing:
                raise hip.SdfError(f"firing-rate monitor: {len(missing)} neuron calls were not recorded by this forward, e.g. {missing[:3]}")
        except BaseException:
            self._table[self._n].zero_()                 # (a forward that failed leaves no record)
            raise
        finally:
            engine.monitor = None
        self._steps.append([s[0] for s in self._seen])
        self._elements.append([s[1] for s in self._seen])
        self._seen = None
        self._n += 1
        return flows

    def _room(self, device):
        """Room for one more forward: the table doubles as FlowMetrics.reserve's does, by a copy on the stream (no synchronisation)."""
        shape = (len(self.names), self.Tmax)
        if self._table is None or self._table.device != device:
            if self._n:
                raise hip.SdfError(f"firing-rate monitor: records so far are on {self._table.device}, this forward on {device}; reset() first")
            self._table = torch.zeros((self._reserve,) + shape, dtype=torch.int64, device=device)
        elif self._n == self._table.shape[0]:
            table = torch.zeros((2 * self._n,) + shape, dtype=torch.int64, device=device)
            table[:self._n] = self._table
            self._table = table

    def record(self, name, spikes, layout):
        """engine._rec's sink: count the u8 spikes of neuron call `name` where they lie.  `layout` is the tape's tag: "flat" has the
        time steps on dim 0, "BDHWC->..." on dim 1."""
        i = self._index.get(name.rstrip("."))
        if i is None:
            raise hip.SdfError(f"firing-rate monitor: the forward recorded {name!r}, which is not a neuron call of this model")
        if self._seen[i] is not None:
            raise hip.SdfError(f"firing-rate monitor: neuron call {name!r} recorded twice in one forward")
        t_dim = 0 if layout == "flat" else 1
        T = spikes.shape[t_dim]
        if T > self.Tmax:
            raise hip.SdfError(f"firing-rate monitor: {name!r} has {T} time steps, the table {self.Tmax}")
        hip.spike_count(spikes, t_dim, counts=self._table[self._n, i, :T])
        self._seen[i] = (T, spikes.numel() // T)

    # ------------------------------------------------------------------ reading
    def counts(self):
        """(forwards, calls, Tmax) int64 on the device: spikes per forward, call and time step; steps beyond a call's T are 0.
        (Reading it synchronises.)"""
        if self._table is None:                          # (nothing recorded yet: an empty table where the model lies)
            return torch.zeros((0, len(self.names), self.Tmax), dtype=torch.int64, device=next(self.model.parameters()).device)
        return self._table[:self._n]

    @property
    def forwards(self):
        return self._n

    @property
    def elements(self):
        """Per call: elements per time step of the reference's tensor at that call (of the last forward)."""
        return list(self._elements[-1]) if self._elements else []

    def _host(self):
        """[forward][call] -> list of T rates (Python floats); ONE synchronising copy of the table."""
        if not self._n:
            return []
        tab = self._table[:self._n].cpu().tolist()
        return [[[c / el for c in tab[f][i][:T]] for i, (T, el) in enumerate(zip(self._steps[f], self._elements[f]))]
                for f in range(self._n)]

    @property
    def records(self):
        """Per forward, per call: the (T,) fp32 rate tensor the reference's monitor holds for that call (synchronises once)."""
        return [[torch.tensor(r, dtype=torch.float32) for r in fwd] for fwd in self._host()]

    def mean(self):
        """Mean over the forwards of the mean over the calls of the mean over the steps: the number the reference prints."""
        rates = self._host()
        if not rates:
            return float("nan")
        return sum(sum(sum(r) / len(r) for r in fwd) / len(fwd) for fwd in rates) / len(rates)

    def rates(self):
        """name -> list of T rates, averaged over the forwards."""
        host = self._host()
        out = {}
        for i, name in enumerate(self.names):
            per = [fwd[i] for fwd in host]
            out[name] = [sum(col) / len(col) for col in zip(*per)] if per else []
        return out

    def to_csv(self, path):
        """Append one row per forward and call: forward index, name, the T rates."""
        host = self._host()
        with open(path, "a", newline="") as f:
            w = csv.writer(f)
            for k, fwd in enumerate(host):
                for name, r in zip(self.names, fwd):
                    w.writerow([k, name] + r)
