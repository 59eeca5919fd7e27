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

`ReplicaFiringRateMonitor` is the same record per SAMPLE of `model.forward_replicas(x[R])` - the launch sequence of the streamed
evaluation (harness.evaluate_stream(..., monitor=)) - counted by one launch per record of the per-sample kernel
(hip.spike_count_samples, csrc/spike_count.hip: sdf_spike_count_seg_fwd), eagerly into its own table or, under graph capture, into a
static count block of the caller's.

The reference's other diagnostic, `vis.monitor_v` (eval_DSEC_flow_SNN.py:145-149, 228-230: `v_seq`, the membrane after reset at every
time step of every neuron call), is `MembraneMonitor` below: the same names, the same switching, the forward on the unfused plan
(engine_unfused.py), per-step statistics in integers on the device (csrc/membrane_stats.hip, restated here in numpy: membrane_record).
One monitor of either kind at a time on a model.
"""
import contextlib
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


# ---------------------------------------------------------------------- the membrane record, restated on the host
# csrc/membrane_stats.hip adds, per time step, [n_nan, sum_q16, min_key, max_key, hist[0 .. bins + 1]] into 64-bit integers.  The same
# arithmetic in numpy - fp32 operations rounded one by one, integers from there on - is what the tests compare the kernel's table with,
# integer for integer, and what the monitor's reading side decodes with.
def membrane_keys(v):
    """Order-preserving unsigned keys of fp32 values: bits ^ (sign ? 0xFFFFFFFF : 0x80000000), as int64."""
    import numpy as np
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return (bits ^ np.where(bits >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))).astype(np.int64)


def membrane_unkey(key):
    """The exact fp32 value (as a numpy float32 array) of membrane_keys' keys."""
    import numpy as np
    key = np.asarray(key, dtype=np.int64).astype(np.uint32)
    return (key ^ np.where(key >> 31, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def membrane_edges(lo, hi, bins):
    """The bins + 1 edges of the histogram's inner bins, float64, from the fp32 bounds the kernel takes."""
    import numpy as np
    lo32, hi32, _ = hip.membrane_inv_width(lo, hi, bins)
    return lo32 + (hi32 - lo32) * np.arange(bins + 1, dtype=np.float64) / bins


def membrane_record(v, lo, hi, bins):
    """v (T, ...) fp32 (numpy) -> the (T, 4 + bins + 2) int64 records sdf_membrane_stats_fwd leaves in a fresh table."""
    import numpy as np
    v = np.ascontiguousarray(v, dtype=np.float32)
    v = v.reshape(v.shape[0], -1)
    lo32, hi32, inv = (np.float32(a) for a in hip.membrane_inv_width(lo, hi, bins))
    table = np.zeros((v.shape[0], hip.MEMBRANE_HEAD + bins + 2), dtype=np.int64)
    table[:, 2] = hip.MEMBRANE_KEY_INIT[0]
    for t, row in enumerate(v):
        nan = np.isnan(row)
        x = row[~nan]
        table[t, 0] = int(nan.sum())
        with np.errstate(over="ignore", invalid="ignore"):
            table[t, 1] = int(np.rint(np.clip(x, np.float32(-32768.0), np.float32(32768.0)) * np.float32(65536.0)).astype(np.int64).sum())
            if x.size:
                keys = membrane_keys(x)
                table[t, 2], table[t, 3] = int(keys.min()), int(keys.max())
            inner = (x >= lo32) & (x < hi32)
            p = (x[inner] - lo32) * inv                                    # (fp32 subtraction, then fp32 product: two roundings)
            idx = 1 + np.minimum(bins - 1, np.floor(p).astype(np.int64))
        hist = np.bincount(idx, minlength=bins + 2)
        hist[0], hist[bins + 1] = int((x < lo32).sum()), int((x >= hi32).sum())
        table[t, hip.MEMBRANE_HEAD:] = hist
    return table


class FiringRateMonitor:
    """Per-step spike counts of every neuron call of `model`'s eval forwards while enabled (see the module's text).  `forwards`: rows
    the count table starts with; it doubles when they run out."""
    what = "firing-rate monitor"      # how the model's refusals name the enabled monitor

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
            raise RuntimeError(f"another {type(other).__name__} is enabled on this model (one monitor at a time: a forward takes one "
                               "recording route): disable() it first")
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

    def _call(self, name, spikes, layout):
        """(index of neuron call `name`, step axis of its record, T), with record()'s refusals."""
        i = self._index.get(name.rstrip("."))
        if i is None:
            raise hip.SdfError(f"firing-rate monitor: the forward recorded {name!r}, which is not a neuron call of this model")
        if self._seen[i] is not None:
            raise hip.SdfError(f"firing-rate monitor: neuron call {name!r} recorded twice in one forward")
        t_dim = 0 if layout == "flat" else 1
        T = spikes.shape[t_dim]
        if T > self.Tmax:
            raise hip.SdfError(f"firing-rate monitor: {name!r} has {T} time steps, the table {self.Tmax}")
        return i, t_dim, T

    def record(self, name, spikes, layout, elements=None):
        """engine._rec's sink: count the u8 spikes of neuron call `name` where they lie.  `layout` is the tape's tag: "flat" has the
        time steps on dim 0, "BDHWC->..." on dim 1.  `elements`: the reference tensor's elements per step where the record is not
        that tensor itself (the patch merging's spikes before the 2x2 concatenation and its zero rows)."""
        i, t_dim, T = self._call(name, spikes, layout)
        hip.spike_count(spikes, t_dim, counts=self._table[self._n, i, :T])
        self._seen[i] = (T, spikes.numel() // T if elements is None else int(elements))

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


class ReplicaFiringRateMonitor(FiringRateMonitor):
    """FiringRateMonitor for the streamed rate: one record set per SAMPLE of `model.forward_replicas(x[R])` (and of `model(x[1])`),
    in sample order, integer for integer what R separate monitored batch-1 forwards count.

        mon = ReplicaFiringRateMonitor(model)
        with mon:
            model.forward_replicas(x)                  # eager: R more rows of the monitor's own table (which may grow)
            with mon.into(block):                      # block (n, calls, Tmax) int64, the caller's and zeroed by the caller
                model.forward_replicas(x[:n])          # ... ADDS its counts into the block instead: what a graph capture records
            mon.take(block, first=k)                   # copy of a filled block into rows k .. k + n of the table, on the current stream
        mon.names, mon.counts(), mon.elements, mon.records, mon.mean(), mon.rates(), mon.to_csv(path)     # as FiringRateMonitor's

    The replica launch sequence takes the engine's recording route with R times the rows; every record is ONE launch of the
    per-sample count kernel (hip.spike_count_samples) on the tensor where it lies: the samples are dim 0 of a channel-last record and
    R equal consecutive pieces of every time block of a window record (engine.MSFlowEngine._rec).  Where `forward_replicas` serves
    its samples one by one (the SEW family, glif, gemm_nsplit != 2, T other than 10 / 20, an odd window count) the monitor does the
    same and sample i's records go to row i.  Under graph capture nothing may be allocated or grown by the monitor and no
    destination may depend on the replay: a capture without a block is refused before the engine is packed; the step counts and
    denominators are host-known at capture and serve every replay of that graph (take).  A reference batch - `model(x[B > 1])` -
    couples its samples and is refused: that is FiringRateMonitor's.  Eval mode, one monitor at a time."""
    what = "replica firing-rate monitor"
    replicas = True                   # what forward_replicas asks an enabled monitor

    def __init__(self, model, forwards=16):
        self._block, self._cur = None, None
        # filled count block -> per sample (steps, elements per step) of every call: host-known when the block was filled, and a
        # property of the (captured) sequence that fills it, not of the records - reset() keeps it
        self._meta = {}
        super().__init__(model, forwards)

    # ------------------------------------------------------------------ the table
    def reserve(self, rows, device=None):
        """Room for `rows` samples in the table.  It grows by a copy on the current stream: a caller whose other streams still write
        into the table (take) lets the current stream wait for them first (harness.StreamEvaluator.run)."""
        shape = (len(self.names), self.Tmax)
        if device is None:
            device = self._table.device if self._table is not None else next(self.model.parameters()).device
        device = torch.device(device)
        if device.index is None and device.type == "cuda":
            device = torch.device("cuda", torch.cuda.current_device())
        if self._table is not None and self._table.device != device:
            if self._n:
                raise hip.SdfError(f"firing-rate monitor: records so far are on {self._table.device}, these on {device}; reset() first")
            self._table = None
        if self._table is None:
            self._table = torch.zeros((max(int(rows), self._reserve),) + shape, dtype=torch.int64, device=device)
        elif rows > self._table.shape[0]:
            table = torch.zeros((max(int(rows), 2 * self._table.shape[0]),) + shape, dtype=torch.int64, device=device)
            table[:self._table.shape[0]] = self._table
            self._table = table
        return self

    @property
    def capacity(self):
        """Samples the table holds without growing."""
        return 0 if self._table is None else self._table.shape[0]

    def _set_row(self, row, steps, elements):
        while len(self._steps) <= row:
            self._steps.append(None)
            self._elements.append(None)
        self._steps[row], self._elements[row] = steps, elements

    def _check_block(self, block):
        shape = (len(self.names), self.Tmax)
        if not (torch.is_tensor(block) and block.is_cuda and block.dtype == torch.int64 and block.dim() == 3 and block.shape[0] >= 1
                and tuple(block.shape[1:]) == shape and block.is_contiguous()):
            raise hip.SdfError(f"replica firing-rate monitor: a count block is a contiguous int64 device tensor (n, {shape[0]}, {shape[1]}) "
                               "- (samples, calls, Tmax)")
        return block

    @contextlib.contextmanager
    def into(self, block):
        """While inside: the monitored forwards ADD their counts into the caller's `block` (n, calls, Tmax) int64 - n = the samples of
        the forward - and leave the table alone; take(block) puts a filled block into the table.  (A launch sequence that
        forward_replicas abandons for the one-by-one route zeroes the rows it had begun: zero the block yourself before the forward.)"""
        prev, self._block = self._block, self._check_block(block)
        try:
            yield self
        finally:
            self._block = prev

    def take(self, block, first=None):
        """Enqueue, on the current stream, the copy of a block filled under into() into rows first .. first + n of the table (default:
        behind the last row); the rows' step counts and denominators are those of the forward that filled the block - of the
        capture, for every replay of a graph.  No synchronisation."""
        meta = self._meta.get((self._check_block(block).data_ptr(), block.shape[0]))
        if meta is None:
            raise hip.SdfError("replica firing-rate monitor: take() of a block that no forward has filled under into()")
        n, k = len(meta), self._n if first is None else int(first)
        if k < 0:
            raise hip.SdfError(f"replica firing-rate monitor: take(first={first})")
        self.reserve(k + n, block.device)
        self._table[k:k + n].copy_(block, non_blocking=True)
        for r, (steps, elements) in enumerate(meta):
            self._set_row(k + r, steps, elements)
        self._n = max(self._n, k + n)
        return self

    # ------------------------------------------------------------------ the forwards (called by the model)
    @contextlib.contextmanager
    def group(self, x):
        """One `forward_replicas(x)` / `model(x[1])`: the refusals first - nothing is packed or launched for a call that is refused -
        then the destination of its x.shape[0] record sets; run() fills them, sample by sample or all at once."""
        if not x.is_cuda:
            raise hip.SdfError("input must be a GPU tensor (no CPU fallback)")
        if self._cur is not None:
            raise RuntimeError("replica firing-rate monitor: a monitored forward is already running on this model")
        R = x.shape[0]
        if self._block is not None:
            if self._block.shape[0] != R or self._block.device != x.device:
                raise hip.SdfError(f"replica firing-rate monitor: the count block holds {self._block.shape[0]} samples on "
                                   f"{self._block.device}, the forward {R} on {x.device}")
            dest = self._block
        elif torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a replica firing-rate monitor is enabled during graph capture without a count block: a captured sequence "
                               "may grow no table and add to no place that depends on the replay - capture under `with mon.into(block)` "
                               "with a static (n, calls, Tmax) int64 block and take() it after every replay, or disable() the monitor")
        else:
            self.reserve(self._n + R, x.device)
            dest = self._table[self._n:self._n + R]
        self._cur = {"dest": dest, "meta": [None] * R}
        try:
            yield self
            meta = self._cur["meta"]
            if any(m is None for m in meta):
                raise hip.SdfError(f"replica firing-rate monitor: {sum(m is None for m in meta)} of {R} samples were not served")
            if self._block is not None:
                self._meta[(dest.data_ptr(), R)] = meta
            else:
                for r, (steps, elements) in enumerate(meta):
                    self._set_row(self._n + r, steps, elements)
                self._n += R
        except BaseException:
            if self._block is None:
                dest.zero_()                             # (a forward that failed leaves no record)
            raise
        finally:
            self._cur = None

    def run(self, engine, x, row=0, replicas=False, scores=None):
        """Inside group(): `engine.forward(x)` on the recording route with its records counted into rows row .. of the group -
        x.shape[0] samples in one launch sequence (`replicas`), else the one sample x (1, ...)."""
        n = x.shape[0]
        if self._cur is None or (not replicas and n != 1) or row + n > len(self._cur["meta"]):
            raise hip.SdfError("replica firing-rate monitor: run() serves the samples of the group() it is called in")
        self._seen, self._row, self._samples = [None] * len(self.names), row, n
        engine.monitor = self
        try:
            flows = engine.forward(x, None, replicas=True) if replicas else engine.forward(x, scores)
            missing = [m for m, s in zip(self.names, self._seen) if s is None]
            if missing:
                raise hip.SdfError(f"firing-rate monitor: {len(missing)} neuron calls were not recorded by this forward, e.g. {missing[:3]}")
        except BaseException:
            self._cur["dest"][row:row + n].zero_()       # (a launch sequence that is abandoned leaves nothing in its rows)
            raise
        finally:
            engine.monitor = None
            seen, self._seen = self._seen, None
        steps, elements = [s[0] for s in seen], [s[1] for s in seen]
        self._cur["meta"][row:row + n] = [(steps, elements)] * n
        return flows

    def forward(self, x, scores=None):
        """`model(x)`: one sample.  A reference batch is refused - its samples are coupled, there is no per-sample record of it."""
        if x.dim() < 1 or x.shape[0] != 1:
            raise RuntimeError(f"a replica firing-rate monitor is enabled and model(x) was called on a batch of {x.shape[0] if x.dim() else 0}: "
                               "a reference batch couples its samples through the window view and has no per-sample record - use "
                               "FiringRateMonitor for a reference batch, or model.forward_replicas(x) for independent samples")
        with self.group(x):
            return self.run(self.model.eval_engine(), x, 0, False, scores)

    def record(self, name, spikes, layout, elements=None, samples=1):
        """engine._rec's sink.  `samples` > 1: the record of a replica launch sequence - one launch of the per-sample kernel, the
        samples outside time ("BDHWC->...": dim 0) or inside it ("flat": equal consecutive pieces of every time block)."""
        i, t_dim, T = self._call(name, spikes, layout)
        if samples != self._samples:
            raise hip.SdfError(f"firing-rate monitor: {name!r} holds {samples} samples, the forward {self._samples}")
        dst = self._cur["dest"][self._row:self._row + samples, i, :T]
        if samples == 1:
            hip.spike_count(spikes, t_dim, counts=dst[0])
        else:
            hip.spike_count_samples(spikes, t_dim, samples, dst)
        self._seen[i] = (T, (spikes.numel() // T if elements is None else int(elements)) // samples)

    # ------------------------------------------------------------------ reading
    def _host(self):
        empty = [k for k in range(self._n) if k >= len(self._steps) or self._steps[k] is None]
        if empty:
            raise hip.SdfError(f"replica firing-rate monitor: rows {empty[:5]} of the table were never filled (take(first=) left a gap)")
        return super()._host()


def membrane_summary(records, elements):
    """Host arithmetic of the membrane monitor, float64: records (forwards, T, 4 + bins + 2) int64 of ONE call (numpy), `elements` per
    step and forward -> {"n_nan" (T,), "mean" (T,), "min" (T,), "max" (T,), "hist" (T, bins + 2)} over the forwards together:
    mean = sum_q16 / 65536 / (elements - n_nan) (good to 2^-17), min / max = the keys decoded back to the exact floats (NaN where a step
    held no number), hist summed."""
    import numpy as np
    records = np.asarray(records, dtype=np.int64)
    n_nan, total = records[:, :, 0].sum(0), records.shape[0] * int(elements)
    count = total - n_nan
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = records[:, :, 1].sum(0).astype(np.float64) / 65536.0 / count
    kmin, kmax = records[:, :, 2].min(0), records[:, :, 3].max(0)
    seen = kmin <= kmax
    lo = np.where(seen, membrane_unkey(np.where(seen, kmin, 0x80000000)).astype(np.float64), np.nan)
    hi = np.where(seen, membrane_unkey(np.where(seen, kmax, 0x80000000)).astype(np.float64), np.nan)
    return {"n_nan": n_nan, "mean": mean, "min": lo, "max": hi, "hist": records[:, :, hip.MEMBRANE_HEAD:].sum(0)}


_TO_REFERENCE = {"flat": None, "BDHWC->TBCHW": (1, 0, 4, 2, 3), "BDHWC->TBHWC": (1, 0, 2, 3, 4)}


class MembraneMonitor(FiringRateMonitor):
    """Per-step membrane statistics of every neuron call of `model`'s eval forwards while enabled: the reference's `vis.monitor_v`
    (eval_DSEC_flow_SNN.py:145-149, 228-230: `store_v_seq = True` on every neuron, `v_seq` - the membrane after reset at every time
    step - recorded per call).

        mon = MembraneMonitor(model, bins=64, range=(-2.0, 2.0), keep=())     # range in multiples of v_th
        with mon: model(x)
        mon.names                  # neuron_call_names(model): shared with the firing-rate monitor
        mon.table()                # (forwards, calls, Tmax, 4 + bins + 2) int64 on the device (csrc/membrane_stats.hip's records)
        mon.elements, mon.mean(), mon.min(), mon.max(), mon.hist(), mon.edges  # one read-back, formed on the host in float64
        mon.v_seq(name)            # names listed in `keep` ("all" allowed): the LAST forward's fp32 membrane in the reference's
                                   # tensor order (the record's layout tag applied) - what `v_seq_monitor.records` holds
        mon.to_csv(path); mon.reset()

    While enabled, the model's eval forward runs on `model.unfused_engine()` (engine_unfused.py): every neuron call allocates a v_seq
    with the spike buffer's addressing, launches `sdf_neuron_vseq_fwd` and one `sdf_membrane_stats_fwd` into this forward's records,
    and releases the buffer unless the call is kept.  The host does not synchronise per forward; the table doubles as the firing-rate
    table does.  The token gate's call `attn.sn2_q` and the dead score `attn.attn_sn` are RECOMPUTED through the general launch
    (engine.MSFlowEngine._rec_gates): the gate's record is a recomputation, not a read-out of the gate kernel.
    MS models with `lif` / `if` / `plif` / `SLTTlif` neurons, eval mode, eager, one forward at a time, one monitor at a time."""
    what = "membrane monitor"

    def __init__(self, model, bins=64, range=(-2.0, 2.0), keep=(), forwards=16):
        from .STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet, SpikingformerFlowNet
        if not isinstance(model, MS_SpikingformerFlowNet):
            raise hip.SdfError(f"MembraneMonitor records membranes: {type(model).__name__} is not a spiking model of this package (the ANN "
                               "model STTFlowNet has no neuron calls); use MS_SpikingformerFlowNet(_en4)")
        if isinstance(model, SpikingformerFlowNet):
            raise hip.SdfError("MembraneMonitor is not built for the SEW family (SpikingformerFlowNet): use an MS model "
                               "(MS_SpikingformerFlowNet(_en4)), or FiringRateMonitor for this model's firing rates")
        kind = model.sttmultires_unet.spiking_kwargs.get("neuron_type")
        if kind in ("psn", "glif"):
            raise hip.SdfError(f"MembraneMonitor: a {kind} neuron keeps no membrane sequence (the reference's node has no v_seq either): "
                               "build the model with lif / if / plif / SLTTlif neurons, or use FiringRateMonitor for its firing rates")
        bins = int(bins)
        if not 1 <= bins <= 256:
            raise hip.SdfError(f"MembraneMonitor: {bins} histogram bins; the statistics kernel takes 1 to 256")
        if not float(range[0]) < float(range[1]):
            raise hip.SdfError(f"MembraneMonitor: range {tuple(range)} is empty; give (lo, hi) in multiples of v_th with lo < hi")
        self.model = model
        self.names = neuron_call_names(model)
        self._index = {n: i for i, n in enumerate(self.names)}
        unet = model.sttmultires_unet
        self.Tmax = max(int(unet.steps), int(unet.window_size[0]))
        if self.Tmax > 64:
            raise hip.SdfError(f"MembraneMonitor: {self.Tmax} time steps; the statistics kernel takes at most 64 - monitor a model "
                               "with fewer steps")
        self.v_th = float(unet.spiking_kwargs["v_th"])
        self.bins, self.lo, self.hi = bins, float(range[0]) * self.v_th, float(range[1]) * self.v_th
        self.edges = membrane_edges(self.lo, self.hi, bins)
        keep = self.names if keep == "all" else [k if k.endswith(_SUFFIX) else k + _SUFFIX for k in ([keep] if isinstance(keep, str) else keep)]
        unknown = [k for k in keep if k not in self._index]
        if unknown:
            raise hip.SdfError(f"MembraneMonitor: keep= names {unknown[:3]}, which are not neuron calls of this model (see .names)")
        self.keep = frozenset(keep)
        self._reserve = max(int(forwards), 1)
        self.reset()

    def reset(self):
        super().reset()
        self._kept = {}

    # ------------------------------------------------------------------ the forward (called by the model)
    def _fresh(self, shape, device):
        table = torch.zeros(tuple(shape) + (hip.MEMBRANE_HEAD + self.bins + 2,), dtype=torch.int64, device=device)
        table[..., 2] = hip.MEMBRANE_KEY_INIT[0]
        return table

    def _room(self, device):
        shape = (len(self.names), self.Tmax)
        if self._table is None or self._table.device != device:
            if self._n:
                raise hip.SdfError(f"membrane monitor: records so far are on {self._table.device}, this forward on {device}; reset() first")
            self._table = self._fresh((self._reserve,) + shape, device)
        elif self._n == self._table.shape[0]:
            table = self._fresh((2 * self._n,) + shape, device)
            table[:self._n] = self._table
            self._table = table

    def forward(self, x, scores=None):
        """One monitored forward on the model's unfused plan.  The refusals come first: nothing is packed or launched for a forward
        that is refused."""
        if not x.is_cuda:
            raise hip.SdfError("input must be a GPU tensor (no CPU fallback)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a membrane monitor is enabled during graph capture: its forward allocates a membrane per neuron call and "
                               "grows a table - disable() the monitor around the capture, or run the monitored forwards eagerly")
        if scores is not None:
            raise NotImplementedError("a membrane monitor is enabled and log=True was asked for: the unfused plan computes no attention "
                                      "score - call model(x) without log, or disable() the monitor")
        engine = self.model.unfused_engine()
        self._room(x.device)
        self._seen, kept = [None] * len(self.names), {}
        engine.monitor, engine._membranes, self._keeping = self, True, kept
        try:
            flows = engine.forward(x)
            missing = [n for n, s in zip(self.names, self._seen) if s is None]
            if missing:
                raise hip.SdfError(f"membrane monitor: {len(missing)} neuron calls were not recorded by this forward, e.g. {missing[:3]}")
        except BaseException:
            self._table[self._n] = self._fresh(self._table.shape[1:3], x.device)      # (a forward that failed leaves no record)
            raise
        finally:
            engine.monitor, engine._membranes, self._keeping = None, False, None
        self._steps.append([s[0] for s in self._seen])
        self._elements.append([s[1] for s in self._seen])
        self._seen, self._kept = None, kept
        self._n += 1
        return flows

    def record(self, name, v, layout):
        """The unfused engine's sink: the statistics of the fp32 membrane `v` of neuron call `name` where it lies, with the spikes'
        own shape, strides and layout tag ("flat": steps on dim 0, "BDHWC->...": on dim 1)."""
        name = name.rstrip(".")
        i = self._index.get(name)
        if i is None:
            raise hip.SdfError(f"membrane monitor: the forward recorded {name!r}, which is not a neuron call of this model")
        if self._seen[i] is not None:
            raise hip.SdfError(f"membrane monitor: neuron call {name!r} recorded twice in one forward")
        if v.dtype != torch.float32:
            raise hip.SdfError(f"membrane monitor: {name!r} handed over {v.dtype}, not its fp32 membrane (is the forward on the unfused plan?)")
        t_dim = 0 if layout == "flat" else 1
        T = v.shape[t_dim]
        if T > self.Tmax:
            raise hip.SdfError(f"membrane monitor: {name!r} has {T} time steps, the table {self.Tmax}")
        hip.membrane_stats(v, t_dim, self._table[self._n, i, :T], self.lo, self.hi, self.bins)
        self._seen[i] = (T, v.numel() // T)
        if name in self.keep:
            self._keeping[name] = (v, layout)

    # ------------------------------------------------------------------ reading
    def table(self):
        """(forwards, calls, Tmax, 4 + bins + 2) int64 on the device: [n_nan, sum_q16, min_key, max_key, hist] per forward, call and
        step; steps beyond a call's T keep their initial record.  (Reading it synchronises.)"""
        if self._table is None:
            return self._fresh((0, len(self.names), self.Tmax), next(self.model.parameters()).device)
        return self._table[:self._n]

    counts = table

    def _host(self):
        """name -> membrane_summary over the forwards; ONE synchronising copy of the table."""
        if not self._n:
            return {}
        tab = self._table[:self._n].cpu().numpy()
        out = {}
        for i, name in enumerate(self.names):
            T, el = self._steps[-1][i], self._elements[-1][i]
            if any(s[i] != T or e[i] != el for s, e in zip(self._steps, self._elements)):
                raise hip.SdfError(f"membrane monitor: {name!r} changed its size between the forwards; reset() between input sizes")
            out[name] = membrane_summary(tab[:, i, :T], el)
        return out

    def mean(self):
        """name -> (T,) float64: the mean membrane per step over the forwards (NaNs left out)."""
        return {n: s["mean"] for n, s in self._host().items()}

    def min(self):
        return {n: s["min"] for n, s in self._host().items()}

    def max(self):
        return {n: s["max"] for n, s in self._host().items()}

    def hist(self):
        """name -> (T, bins + 2) int64 summed over the forwards: underflow, the bins between .edges, overflow."""
        return {n: s["hist"] for n, s in self._host().items()}

    def summary(self):
        """name -> {"mean", "min", "max": T floats, "hist": T lists of bins + 2 counts, "n_nan": T counts} as plain Python values."""
        return {n: {k: v.tolist() for k, v in s.items()} for n, s in self._host().items()}

    records = property(lambda self: self.summary())
    rates = summary

    def v_seq(self, name):
        """The last forward's fp32 membrane of a kept call in the reference's tensor order (time steps first)."""
        name = name if name.endswith(_SUFFIX) else name + _SUFFIX
        if name not in self._kept:
            raise hip.SdfError(f"membrane monitor: no membrane kept for {name!r}: list it in keep= (or keep='all') and run a forward")
        v, layout = self._kept[name]
        perm = _TO_REFERENCE[layout]
        return v if perm is None else v.permute(*perm)

    def to_csv(self, path):
        """Append one row per forward, call and step: forward, name, step, elements, n_nan, mean, min, max, the bins + 2 counts."""
        if not self._n:
            return
        tab = self._table[:self._n].cpu().numpy()
        with open(path, "a", newline="") as f:
            w = csv.writer(f)
            for k in range(self._n):
                for i, name in enumerate(self.names):
                    T, el = self._steps[k][i], self._elements[k][i]
                    s = membrane_summary(tab[k:k + 1, i, :T], el)
                    for t in range(T):
                        w.writerow([k, name, t, el, int(s["n_nan"][t]), repr(float(s["mean"][t])), repr(float(s["min"][t])),
                                    repr(float(s["max"][t]))] + s["hist"][t].tolist())
