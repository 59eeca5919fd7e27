"""The model-facing steps of the reference's evaluation loop (eval_DSEC_flow_SNN.valid_test :153-271),
restated so that the harness logic runs with this package: input preparation, forward, metric accumulation.
Dataset loading, MLflow and visualisation are out of scope."""
import torch
import torch.nn.functional as F


def center_crop(t, size):
    """Centre crop of the last two dims (reference DSEC_dataloader/data_augmentation.py:62-86)."""
    H, W = t.shape[-2:]
    th, tw = size
    i, j = (H - th) // 2, (W - tw) // 2
    return t[..., i:i + th, j:j + tw]


def prepare_chunk(voxel, norm_input="minmax", spike_th=None, polarity=True):
    """signed voxel (B,bins,H,W) -> network input (B,bins,2,H,W).

    pos/neg split stacked on dim 2 (eval_DSEC_flow_SNN.py:179-186), min-max over the non-zeros of the
    WHOLE batch tensor (:199-205) or mean/std (:206-212), optional binarisation (:215-217)."""
    chunk = torch.stack((F.relu(voxel), F.relu(-voxel)), dim=2) if polarity else voxel
    nz = chunk != 0
    if nz.any():
        vals = chunk[nz]
        if norm_input == "minmax":
            lo, hi = vals.min(), vals.max()
            if lo != hi:
                chunk = torch.where(nz, (chunk - lo) / (hi - lo), chunk)
        elif norm_input == "std":
            mean, std = vals.mean(), vals.std()
            if std > 0:
                chunk = torch.where(nz, (chunk - mean) / std, chunk)
    if spike_th is not None:
        chunk = torch.where(chunk > spike_th, torch.ones_like(chunk), torch.where(chunk < spike_th, torch.zeros_like(chunk), chunk))
    return chunk


def event_times(ts):
    """Integer sensor timestamps -> the fp32 times the voxeliser takes, as the reference's preprocessing forms them
    (DSEC_dataset_preprocess.py:185-186): (t - t[0]) in integers, to fp32, divided by the last.  Floating times pass as fp32."""
    if ts.is_floating_point() or ts.numel() == 0:
        return ts.to(torch.float32)
    t = (ts - ts[0]).to(torch.float32)
    return t / t[-1]


def _event_columns(events, rectify_map, times):
    """One event dict, or a list of B of them, as the back-to-back arrays the event kernels take: x, y (fp32 - or int32 / uint16 with a
    `rectify_map`), t (`times` of each list's 't' or 'ts'), p (fp32) and the B + 1 list offsets.  Host tensors are refused."""
    from . import hip
    lists = [events] if isinstance(events, dict) else list(events)
    cols = {k: [] for k in "xytp"}
    offsets = [0]
    for ev in lists:
        t = ev["t"] if "t" in ev else ev["ts"]
        for a in (ev["x"], ev["y"], t, ev["p"]):
            if not a.is_cuda:
                raise hip.SdfError("HIP path needs device tensors (no CPU fallback)")
        x, y = ev["x"], ev["y"]
        if rectify_map is not None and x.dtype not in (torch.int32, torch.uint16):
            x, y = x.to(torch.int32), y.to(torch.int32)
        elif rectify_map is None:
            x, y = x.to(torch.float32), y.to(torch.float32)
        for k, a in zip("xytp", (x, y, times(t), ev["p"].to(torch.float32))):
            cols[k].append(a.reshape(-1))
        offsets.append(offsets[-1] + cols["t"][-1].numel())
    return (*(c[0] if len(c) == 1 else torch.cat(c) for c in (cols[k] for k in "xytp")), offsets)


def events_to_chunk(events, bins, sensor_size, crop, norm_input, spike_th, rectify_map=None):
    """Raw events -> network input (B, bins, 2, h, w) in one HIP launch sequence (hip.event_voxel): voxel grid with the reference's
    semantics (event_representations.py:248-277), centre crop, polarity split, normalisation and spike threshold as
    prepare_chunk(center_crop(grid)) gives them, bit for bit.  `events`: a dict of device tensors 'x', 'y', 'p' and 't' (or 'ts'), or a
    list of B such dicts (one batch; min-max runs over the whole batch tensor, as prepare_chunk does).  x, y: fp32, or integer sensor
    coordinates with `rectify_map` (H_s, W_s, 2).  norm_input "std" runs prepare_chunk's own code on the un-normalised output."""
    from . import hip
    x, y, t, p, offsets = _event_columns(events, rectify_map, event_times)
    fused = norm_input if norm_input == "minmax" else None
    chunk = hip.event_voxel(x, y, t, p, bins, tuple(sensor_size), offsets=offsets, crop=tuple(crop) if crop else None, mode="split",
                            norm=fused, spike_th=spike_th if norm_input != "std" else None, rectify_map=rectify_map)
    if norm_input == "std":
        chunk = prepare_chunk(chunk, "std", spike_th, polarity=False)
    return chunk


def center_crop_origin(size, crop):
    """torchvision.transforms.CenterCrop's origin, int(round((H - h) / 2.0)) per axis: (2, 45) for 260 x 346 cropped to 256 x 256."""
    return tuple(int(round((s - c) / 2.0)) for s, c in zip(size, crop))


def event_pairs_to_chunk(pairs, num_frames, sensor_size, crop, norm_input, spike_th, crop_origin=None, want_event_mask=False,
                         timestamp_multiplier=1e6, normalize=True, num_chunks=2):
    """Raw (old, new) event lists -> network input (B, 2 num_frames, 2, h, w) in one HIP launch sequence (hip.event_voxel_tb): per list
    the reference's EventSequence(..., timestamp_multiplier, convert_to_relative=True) and EventSequenceToVoxelGrid_Pytorch
    (MDR_dataloader/loader_utils.py:344-389, 421-577) with its per-list normalisation, the crop window (h, w) at `crop_origin` (default
    torchvision CenterCrop's), then eval_MV_flow_SNN.py:162-213: old | new along the bins, polarity split, normalisation, spike
    threshold - as prepare_chunk(cat(old, new)) gives them, bit for bit.  `pairs`: one (events_old, events_new) pair or a list of B of
    them (min-max runs over the whole batch tensor); each a dict of device tensors 'ts' (or 't', float64), 'x', 'y', 'p'.
    `want_event_mask`: also returns the loop's event mask (:217-219) as fp32 (B, 1, h, w).  norm_input "std" runs prepare_chunk's own
    code on the un-normalised output.  num_chunks 1: only the new list of each pair is used (B, num_frames, 2, h, w)."""
    from . import hip
    if isinstance(pairs, tuple) and len(pairs) == 2 and isinstance(pairs[0], dict):
        pairs = [pairs]
    cols = {k: [] for k in "xytp"}
    offsets = [0]
    for pair in pairs:
        for ev in (pair if num_chunks == 2 else pair[1:]):
            t = ev["ts"] if "ts" in ev else ev["t"]
            x, y, p = ev["x"], ev["y"], ev["p"]
            for a in (x, y, t, p):
                if not a.is_cuda:
                    raise hip.SdfError("HIP path needs device tensors (no CPU fallback)")
            if x.dtype not in (torch.float32, torch.int32, torch.uint16) or y.dtype != x.dtype:
                x, y = x.to(torch.int32), y.to(torch.int32)                 # (.long(): truncation toward zero)
            for k, a in zip("xytp", (x, y, t.to(torch.float64), p.to(torch.float32))):
                cols[k].append(a.reshape(-1))
            offsets.append(offsets[-1] + cols["t"][-1].numel())
    x, y, t, p = (c[0] if len(c) == 1 else torch.cat(c) for c in (cols[k] for k in "xytp"))
    fused = norm_input != "std"
    out = hip.event_voxel_tb(x, y, t, p, num_frames, tuple(sensor_size), offsets=offsets, t_scale=timestamp_multiplier,
                             crop=tuple(crop) if crop else None, crop_origin=crop_origin, normalize=normalize, mode="split",
                             lists_per_sample=num_chunks, norm="minmax" if norm_input == "minmax" else None,
                             spike_th=spike_th if fused else None, want_event_mask=want_event_mask and fused)
    if fused:
        return out
    chunk = prepare_chunk(out, "std", spike_th, polarity=False)
    return (chunk, chunk.sum(1).sum(1, keepdim=True).bool().float()) if want_event_mask else chunk


def warp_times(ts):
    """A list's timestamps -> the fp32 times hip.event_iwe takes.  Integer sensor timestamps and fp32 times: event_times.  The MV
    loaders' float64 seconds: the normalised time (t - t[0]) / (t[-1] - t[0]) is formed in float64 first, so that the microseconds of
    a long recording survive the cast (a list whose times are all equal stays all equal, and is refused as such)."""
    if ts.dtype != torch.float64 or ts.numel() == 0:
        return event_times(ts)
    t = ts - ts[0]
    return torch.where(t[-1] != 0, t / t[-1], t).to(torch.float32)


def warp_events(events, flow, sensor_size, crop, scale, crop_origin=None, t_ref=1.0, window=(0.0, 1.0), mode="bilinear",
                rectify_map=None, check=True):
    """Raw events + an estimated flow -> the image of warped events (B, 2, h, w) in one HIP launch sequence (hip.event_iwe): every event
    moved along `scale` * flow to the time `t_ref` of its normalised window and accumulated per polarity (channel 0: p > 0).
    `events`: a dict of device tensors 'x', 'y', 'p' and 't' (or 'ts'), or a list of B such dicts, as events_to_chunk takes them; flow
    (B, 2, h, w) on the window `crop` (h, w) of `sensor_size` at `crop_origin` (default center_crop's; the MV loops pass
    center_crop_origin's).  x, y: fp32 (other dtypes are cast), or integer sensor coordinates with `rectify_map`.  No backward pass."""
    from . import hip
    x, y, t, p, offsets = _event_columns(events, rectify_map, warp_times)
    return hip.event_iwe(x, y, t, p, flow, tuple(sensor_size), offsets=offsets, crop=tuple(crop) if crop else None,
                         crop_origin=crop_origin, scale=scale, t_ref=t_ref, window=window, mode=mode, rectify_map=rectify_map, check=check)


class _FlowWarp:
    """`fwl=True` of the two loops: every raw-event sample's FWL into a loss.flow_warp.FlowWarpMetrics (read once, at the end) and, when
    the loop stores (`vis.store`), its bilinear image of warped events as <sequence>/iwe/%09d.png beside the other images."""

    def __init__(self, device, window):
        from .loss.flow_warp import FlowWarpMetrics
        self.metrics, self.window = FlowWarpMetrics(64, device), tuple(window)

    @staticmethod
    def needs_events(sample_has_events):
        if not sample_has_events:
            raise ValueError("fwl=True: the warp needs the event list, and this sample came as a voxel tensor - pass the raw events "
                             "(data.preprocessed: false / 'events_new'), or evaluate without fwl")

    def __call__(self, events, pred, size, crop, scale, store, crop_origin=None):
        self.metrics.update(pred, events, size, crop, scale, self.window, crop_origin=crop_origin)
        if store is not None:
            store.iwe(warp_events(events, pred, size, crop, scale, crop_origin=crop_origin, window=self.window, check=False))


def _with_fwl(loop, fwl, fwl_window, device):
    """`loop` with its `warp=` bound and "FWL" (the mean over the samples) added to its dict when `fwl` is true; else `loop`."""
    if not fwl:
        return loop

    def run(model, samples, config, device=device, **kw):
        warp = _FlowWarp(device, fwl_window)
        result = loop(model, samples, config, device, warp=warp, **kw)
        result["FWL"] = warp.metrics.result()["FWL"]
        return result
    return run


def _with_firing_rates(loop, model, samples, config, device, monitor):
    """`loop(model, samples, config, device)` - and, when `vis.monitor_fr` is true (the reference's key, eval_DSEC_flow_SNN.py:140-143),
    its forwards under a monitor.FiringRateMonitor (the caller's `monitor`, or a new one; left as enabled or disabled as it came) and
    two more entries in the dict: "firing_rate" (what the reference prints, :223-227) and "firing_rates" (call name -> its T rates,
    averaged over the forwards).  Key false or absent: the loop alone.
    `vis.monitor_v` true (the reference's other key, :145-149, 228-230): the same under a monitor.MembraneMonitor, and ONE more entry,
    "membrane": call name -> {"mean", "min", "max": T floats, "hist": T lists of bins + 2 counts, "n_nan"} over the forwards (mean
    averaged, extremes over all, histogram summed; the bin edges are the monitor's `.edges`).  Both keys true is refused: a forward
    takes one recording route."""
    vis = config.get("vis") or {}
    want_fr, want_v = bool(vis.get("monitor_fr")), bool(vis.get("monitor_v"))
    if want_fr and want_v:
        raise RuntimeError("vis.monitor_fr and vis.monitor_v are both set: one monitor at a time (the rates are counted on the fused "
                           "plan's recording route, the membranes kept on the unfused plan) - run the evaluation once per key")
    if not (want_fr or want_v):
        return loop(model, samples, config, device)
    from .monitor import FiringRateMonitor, MembraneMonitor
    cls = MembraneMonitor if want_v else FiringRateMonitor
    if monitor is None:
        monitor = cls(model)
    elif monitor.model is not model:
        raise ValueError(f"monitor= belongs to another model: it would record nothing here - pass a {cls.__name__} of this model, or none")
    elif type(monitor) is not cls:
        raise ValueError(f"monitor= is a {type(monitor).__name__}, vis.monitor_{'v' if want_v else 'fr'} asks for a {cls.__name__}: pass one, or none")
    was_on = monitor.enabled
    monitor.enable()
    try:
        result = loop(model, samples, config, device)
    finally:
        if not was_on:
            monitor.disable()
    if want_v:
        result["membrane"] = monitor.summary()
    else:
        result["firing_rate"], result["firing_rates"] = monitor.mean(), monitor.rates()
    return result


class _Storer:
    """`vis.store` of the two loops (the reference's key, eval_DSEC_flow_SNN.py:278-280, eval_MV_flow_SNN.py:256-258): every sample's
    event image, flow and ground-truth flow - and, with `submission`, the flow in the DSEC benchmark's 16-bit encoding - through
    utils.visualization.Visualization_DSEC into <store_dir>/results/eval_0/<sequence>/... (flow_test/<sequence>/ for the submission)."""

    def __init__(self, config, store_dir, sequence, submission):
        from .utils.visualization import Visualization_DSEC
        self.vis = Visualization_DSEC(config, eval_id=0, path_results=store_dir)
        self.sequence, self.submission, self.count = sequence, bool(submission), 0

    def __call__(self, source, label, pred, mask=None):
        """`source`: the signed voxel (B, bins, h, w) on the scored window ("signed" sums) or the model's input (B, bins, 2, h, w)
        ("split" sums: of the NORMALISED input); `mask`: multiplied into both flows first (the MV loop's), None: stored as they are."""
        from . import hip
        if mask is not None:
            label, pred = label * mask, pred * mask
        self.vis.store(hip.event_counts(source), label, mask, pred, self.sequence, flow_test=pred if self.submission else None,
                       idx=self.count)
        self.count += pred.shape[0]

    def iwe(self, image):
        """The image of warped events (B, 2, h, w) of the samples stored last, rendered with the event image's colours, as
        <sequence>/iwe/%09d.png under their numbers."""
        import os
        from . import hip
        from .utils.png import write_png
        path_to = os.path.join(self.vis.store_dir, self.sequence, "iwe")
        os.makedirs(path_to, exist_ok=True)
        host = hip.event_counts_image(image).cpu().numpy()
        for b in range(host.shape[0]):
            write_png(os.path.join(path_to, "%09d.png" % (self.count - host.shape[0] + b)), host[b])


def _storing(loop, config, store_dir, sequence, submission):
    """`loop` with its `store=` bound when `vis.store` is true (refused without a `store_dir`, before any forward); else `loop`."""
    if not (config.get("vis") or {}).get("store"):
        return loop
    if store_dir is None:
        raise ValueError("vis.store is set: pass store_dir= (the images go to <store_dir>/results/eval_0/<sequence>/), or clear the key")
    store = _Storer(config, store_dir, sequence, submission)
    return lambda model, samples, config, device: loop(model, samples, config, device, store=store)


def evaluate_mv(model, samples, config, device="cuda", monitor=None, store_dir=None, sequence="eval", submission=False, fwl=False,
                fwl_window=(0.0, 1.0)):
    """harness.evaluate's counterpart for the MVSEC / MDR sample dicts (`_evaluate_mv`: the loop itself); `vis.monitor_fr` true: the
    forwards run under a FiringRateMonitor (`monitor`, or a new one) and the dict also has "firing_rate" and "firing_rates".
    `vis.store` true: every sample's events, flow * mask and label * mask are stored as harness.evaluate stores them (`store_dir`,
    `sequence`, `submission`).
    `fwl` true: every sample that came as raw events also gets its Flow Warp Loss on 'events_new' (loss.flow_warp), the dict gains
    "FWL", and a storing loop also writes the bilinear image of warped events to <sequence>/iwe/; a voxel sample raises ValueError."""
    loop = _with_fwl(_evaluate_mv, fwl, fwl_window, device)
    return _with_firing_rates(_storing(loop, config, store_dir, sequence, submission), model, samples, config, device, monitor)


def _evaluate_mv(model, samples, config, device="cuda", store=None, warp=None):
    """The model-facing loop of eval_MV_flow_SNN.py:157-249 over an iterable of sample dicts, either the reference loader's
    ('event_volume_old', 'event_volume_new' (B, num_frames, h, w), 'flow' (B, 2, h, w), 'valid' (B, h, w)) or the raw form
    ('events_old', 'events_new': event dicts, or lists of B of them; 'flow', 'valid' at the sensor's or the crop's size, with or without
    the batch dim), which goes through event_pairs_to_chunk at loader.resolution / loader.crop / data.num_frames on the device only.
    Honours data.num_chunks, loader.polarity, model.norm_input, data.spike_th and metrics.mask_events; returns the running means of
    metrics.name: AEE (with PE1-3 and outliers) and AAE."""
    from .loss import flow_supervised
    from .spikingjelly_compat import functional
    names = config["metrics"].get("name", ["AEE", "AAE"])
    chunks = config["data"].get("num_chunks", 2)
    polarity = config["loader"].get("polarity", True)
    norm_input, spike_th = config["model"].get("norm_input"), config["data"].get("spike_th")
    mask_events = config["metrics"].get("mask_events")
    tot = {k: 0.0 for n in names for k in ((n, "PE1", "PE2", "PE3", "outliers") if n == "AEE" else (n,))}
    it = 0
    for data in samples:
        functional.reset_net(model)
        label = data["flow"].to(device, torch.float32)
        mask = data["valid"].to(device, torch.float32)
        if label.dim() == 3:
            label, mask = label.unsqueeze(0), mask.unsqueeze(0)
        mask = mask.unsqueeze(1)
        event_mask = None
        if warp is not None:
            warp.needs_events("events_new" in data)
        if "events_new" in data:
            if not polarity:
                raise ValueError("the event path builds the two-polarity input (loader.polarity: true)")
            old, new = data["events_old"], data["events_new"]
            pairs = [(old, new)] if isinstance(new, dict) else list(zip(old, new))
            pairs = [tuple({k: v.to(device) for k, v in ev.items()} for ev in pair) for pair in pairs]
            size, crop = tuple(config["loader"]["resolution"]), config["loader"].get("crop")
            x = event_pairs_to_chunk(pairs, config["data"]["num_frames"], size, crop, norm_input, spike_th,
                                     want_event_mask=bool(mask_events), num_chunks=chunks)
            if mask_events:
                x, event_mask = x
            if crop and tuple(label.shape[-2:]) == size:
                oy, ox = center_crop_origin(size, crop)
                label, mask = label[..., oy:oy + crop[0], ox:ox + crop[1]], mask[..., oy:oy + crop[0], ox:ox + crop[1]]
        else:
            chunk = data["event_volume_new"].to(device, torch.float32)
            if chunks == 2:
                chunk = torch.cat((data["event_volume_old"].to(device, torch.float32), chunk), dim=1)
            x = prepare_chunk(chunk, norm_input, spike_th, polarity)
            if mask_events:
                event_mask = x.sum(1).sum(1, keepdim=True).bool() if polarity else x.sum(1, keepdim=True).bool()
        with torch.no_grad():
            pred = model(x)["flow"][-1]
        if mask_events:
            mask = mask * event_mask
        if store is not None:
            store(x if "events_new" in data else chunk, label, pred, mask)
        if warp is not None:
            warp([new for _, new in pairs], pred, size, crop, config["metrics"]["flow_scaling"], store,
                 crop_origin=center_crop_origin(size, crop) if crop else None)
        results = {n: getattr(flow_supervised, n)(pred, label, mask, config["metrics"]["flow_scaling"])() for n in names}
        for b in range(pred.shape[0]):
            it += 1
            for n, m in results.items():
                if n == "AEE":
                    tot["AEE"] += float(m[0][b])
                    for key, v in zip(("PE1", "PE2", "PE3", "outliers"), m[1:]):
                        tot[key] += float(v.reshape(-1)[b] if v.numel() > 1 else v)
                else:
                    tot[n] += float(m[0].reshape(-1)[b] if m[0].numel() > 1 else m[0])
    return {k: v / max(it, 1) for k, v in tot.items()}


def evaluate(model, samples, config, device="cuda", monitor=None, store_dir=None, sequence="eval", submission=False, fwl=False,
             fwl_window=(0.0, 1.0)):
    """The evaluation loop (`_evaluate`); `vis.monitor_fr` true: its forwards run under a FiringRateMonitor (`monitor`, or a new one) and
    the dict also has "firing_rate" (its mean()) and "firing_rates" (name -> T rates averaged over the forwards); false or absent:
    nothing changes.
    `vis.store` true (the reference's key): every sample's event image, flow and ground-truth flow, unmasked as the reference stores
    them, are rendered on the GPU and written as PNGs to <store_dir>/results/eval_0/<sequence>/{events, flow, gtflow}/%09d.png, and with
    `submission` the flow in the DSEC benchmark's 16-bit encoding to .../flow_test/<sequence>/%06d.png (utils.visualization); without
    a `store_dir` the key is refused before any forward.  False or absent: nothing changes and no render kernel is launched.
    `vis.enabled` (the live window) is ignored.
    `fwl` true: flow quality without ground truth - every sample that came as raw events also gets its Flow Warp Loss
    (loss.flow_warp: variance of the events warped by the flow over the variance of the unwarped ones, on the events of `fwl_window`
    of the normalised time) and the dict gains "FWL", their mean; a storing loop also writes the bilinear image of warped events to
    .../<sequence>/iwe/%09d.png.  A sample that came as a voxel tensor raises ValueError: the warp needs the event list.  False, the
    default: nothing changes and no warp kernel is launched.  evaluate_stream does not take it: the warp is not built under the
    throughput scheme."""
    loop = _with_fwl(_evaluate, fwl, fwl_window, device)
    return _with_firing_rates(_storing(loop, config, store_dir, sequence, submission), model, samples, config, device, monitor)


def _evaluate(model, samples, config, device="cuda", store=None, warp=None):
    """Run `model` over an iterable of (chunk (B,bins,H,W), mask (B,H,W), label (B,2,H,W)) like
    valid_test does and return the running-mean metrics dict (AEE, PE1-3, outliers) (:253-271, :283-305).
    `chunk` may also be the raw event dict {'ts', 'x', 'y', 'p'} DSECDatasetLite yields when data.preprocessed is false (one sample;
    mask (H,W), label (2,H,W)): it goes through events_to_chunk at loader.resolution / model.num_bins, on the device only."""
    from .loss.flow_supervised import AEE
    from .spikingjelly_compat import functional
    crop = config["loader"].get("crop")
    tot = {"AEE": 0.0, "PE1": 0.0, "PE2": 0.0, "PE3": 0.0, "outliers": 0.0}
    it = 0
    for chunk, mask, label in samples:
        if warp is not None:
            warp.needs_events(isinstance(chunk, dict))
        if isinstance(chunk, dict):
            if not config["loader"].get("polarity", True):
                raise ValueError("the event path builds the two-polarity input (loader.polarity: true)")
            ev = {k: v.to(device) for k, v in chunk.items()}
            x = events_to_chunk(ev, config["model"]["num_bins"], config["loader"]["resolution"], crop,
                                config["model"].get("norm_input"), config["data"].get("spike_th"))
            if label.dim() == 3:
                label, mask = label.unsqueeze(0), mask.unsqueeze(0)
            chunk = None
        functional.reset_net(model)
        label = label.to(device, torch.float32)
        mask = mask.to(device).unsqueeze(1).float()
        if chunk is not None:
            chunk = chunk.to(device, torch.float32)
        if crop:
            label, mask = center_crop(label, crop), center_crop(mask, crop)
        if chunk is not None:
            if crop:
                chunk = center_crop(chunk, crop)
            x = prepare_chunk(chunk, config["model"].get("norm_input"), config["data"].get("spike_th"),
                              config["loader"].get("polarity", True))
        with torch.no_grad():
            pred = model(x)["flow"][-1]
        if config["metrics"].get("mask_events"):
            mask = mask * x.sum(1).sum(1, keepdim=True).bool()
        if store is not None:
            store(x if chunk is None else chunk, label, pred)
        if warp is not None:
            warp(ev, pred, config["loader"]["resolution"], crop, config["metrics"]["flow_scaling"], store)
        m = AEE(pred, label, mask, config["metrics"]["flow_scaling"])()
        for b in range(pred.shape[0]):
            it += 1
            tot["AEE"] += float(m[0][b])
            for key, v in zip(("PE1", "PE2", "PE3", "outliers"), m[1:]):
                tot[key] += float(v.reshape(-1)[b] if v.numel() > 1 else v)
    return {k: v / max(it, 1) for k, v in tot.items()}


def deal(items, streams, replicas):
    """The items of an iterable, in iteration order, cut into groups of `replicas` (the last one may be smaller), the groups dealt
    round-robin to the streams: yields (stream, index of the group's first item, [items])."""
    group, first, g = [], 0, 0
    for item in items:
        group.append(item)
        if len(group) == replicas:
            yield g % streams, first, group
            first, g, group = first + len(group), g + 1, []
    if group:
        yield g % streams, first, group


def stream_plan(n, streams, replicas):
    """How evaluate_stream serves n samples: [(stream, first sample, samples)] in issue order."""
    return [(j, k, len(group)) for j, k, group in deal(range(n), streams, replicas)]


class StreamEvaluator:
    """The execution scheme of the throughput benchmark as a library call: every sample is a batch-1 evaluation, `replicas` of them go
    through ONE launch sequence (model.forward_replicas: bit-equal to separate batch-1 forwards), captured as a HIP graph per stream
    and replayed on `streams` streams; input preparation, metrics (loss.flow_supervised.FlowMetrics) and the optional copy of the flow
    map are enqueued on the group's stream, and the host synchronises once, when run() forms the result.  An instance keeps its static
    buffers and graphs between run() calls; `metrics` is the FlowMetrics of the last run (counts(): the raw per-sample table).
    `monitor`: a monitor.ReplicaFiringRateMonitor of the model - the launch sequences then take the recording route and every sample's
    spike counts go to the monitor's table, row = the sample's index (behind the rows the monitor held before the run)."""

    def __init__(self, model, config, device="cuda", replicas=10, streams=2, graphs=True, monitor=None):
        if replicas < 1 or streams < 1:
            raise ValueError("replicas and streams are at least 1")
        if monitor is not None:
            from .monitor import ReplicaFiringRateMonitor
            if not isinstance(monitor, ReplicaFiringRateMonitor):
                raise TypeError(f"monitor= is a {type(monitor).__name__}: it records single eager forwards (harness.evaluate / evaluate_mv) - "
                                "the streamed evaluation counts per sample under replicas: pass a monitor.ReplicaFiringRateMonitor")
            if monitor.model is not model:
                raise ValueError("monitor= belongs to another model: it would record nothing here - pass a ReplicaFiringRateMonitor of this model")
        elif (config.get("vis") or {}).get("monitor_fr"):
            raise RuntimeError("vis.monitor_fr is set: that key's monitor counts single eager forwards, not replicas and captured graphs - "
                               "use harness.evaluate / evaluate_mv for it, or clear the key and pass monitor=ReplicaFiringRateMonitor(model) "
                               "for the rates at the throughput scheme's rate")
        if (config.get("vis") or {}).get("store"):
            raise RuntimeError("vis.store is set: files are written by harness.evaluate / evaluate_mv (store_dir=) - under the throughput "
                               "scheme pass renders_out= to run() for the rendered bytes on the device, and clear the key")
        if (config.get("vis") or {}).get("monitor_v"):
            raise RuntimeError("vis.monitor_v is set: membranes are recorded on single eager forwards of the unfused plan, not under "
                               "replicas and captured graphs - use harness.evaluate / evaluate_mv, or clear the key for the throughput scheme")
        self.model, self.config, self.device = model, config, torch.device(device)
        self.R, self.F, self.graphs = int(replicas), int(streams), bool(graphs)
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(self.F)]
        self.slots = [None] * self.F                             # per stream: static buffers and {samples: [graph, flow]}
        self.metrics = None
        self.monitor = monitor                                   # a monitor.ReplicaFiringRateMonitor, or None
        self.polarity = config["loader"].get("polarity", True)
        self.norm_input, self.spike_th = config["model"].get("norm_input"), config["data"].get("spike_th")
        self.mask_events = bool(config["metrics"].get("mask_events"))
        self.crop = tuple(config["loader"]["crop"]) if config["loader"].get("crop") else None

    # -- samples -------------------------------------------------------------------------------------------------------------------
    def _units(self, samples):
        """Every sample of every loader item as (kind, payload, label (1, 2, ., .), mask (1, 1, ., .)), label and mask still uncropped
        and wherever the loader left them; kind: 'voxel' (signed volume (1, bins, Hs, Ws), cropped when prepared), 'events' (one event
        dict), 'volume' (old | new volumes, no crop), 'pairs' (one (old, new) pair of event dicts)."""
        chunks = self.config["data"].get("num_chunks", 2)
        for item in samples:
            if isinstance(item, dict):
                label, mask = item["flow"], item["valid"]
                if label.dim() == 3:
                    label, mask = label.unsqueeze(0), mask.unsqueeze(0)
                mask = mask.reshape(mask.shape[0], 1, *mask.shape[-2:])
                if "events_new" in item:
                    old, new = item["events_old"], item["events_new"]
                    pairs = [(old, new)] if isinstance(new, dict) else list(zip(old, new))
                    for b, pair in enumerate(pairs):
                        yield "pairs", pair, label[b:b + 1], mask[b:b + 1]
                else:
                    vol = item["event_volume_new"]
                    if chunks == 2:
                        vol = torch.cat((item["event_volume_old"], vol), dim=1)
                    for b in range(vol.shape[0]):
                        yield "volume", vol[b:b + 1], label[b:b + 1], mask[b:b + 1]
            else:
                chunk, mask, label = item
                if isinstance(chunk, dict):
                    if label.dim() == 3:
                        label, mask = label.unsqueeze(0), mask.unsqueeze(0)
                    yield "events", chunk, label, mask.reshape(1, 1, *mask.shape[-2:])
                else:
                    for b in range(chunk.shape[0]):
                        yield "voxel", chunk[b:b + 1], label[b:b + 1], mask[b:b + 1].reshape(1, 1, *mask.shape[-2:])

    def _window(self, kind, label):
        """(oy, ox, h, w) of the label / mask window the sample is scored on."""
        H, W = label.shape[-2:]
        if not self.crop or kind == "volume":
            return 0, 0, H, W
        h, w = self.crop
        if kind == "pairs":
            size = tuple(self.config["loader"]["resolution"])
            oy, ox = center_crop_origin(size, self.crop) if (H, W) == size else (0, 0)
            return oy, ox, (h if (H, W) == size else H), (w if (H, W) == size else W)
        return (H - h) // 2, (W - w) // 2, h, w

    def _input_shape(self, kind, payload, hw):
        if kind in ("voxel", "volume"):
            bins = payload.shape[1]
        elif kind == "events":
            bins = self.config["model"]["num_bins"]
        else:
            bins = self.config["data"]["num_frames"] * self.config["data"].get("num_chunks", 2)
        return (bins, 2) + hw if self.polarity else (bins,) + hw

    def _prepare(self, kind, payload, x, em):
        """The model's input of one sample into x (1, ...), its event mask into em (1, 1, h, w) when asked - on the current stream."""
        from . import hip
        dev, cfg = self.device, self.config
        if kind in ("events", "pairs") and not self.polarity:
            raise ValueError("the event path builds the two-polarity input (loader.polarity: true)")
        if kind in ("voxel", "volume"):
            v = payload.to(dev, torch.float32)
            crop = self.crop if kind == "voxel" else None
            if self.polarity and self.norm_input != "std":
                hip.prepare_chunk(v, crop, self.norm_input, self.spike_th, out=x, event_mask=em)
                return
            got = prepare_chunk(center_crop(v, crop) if crop else v, self.norm_input, self.spike_th, self.polarity)
        elif kind == "events":
            ev = {k: t.to(dev) for k, t in payload.items()}
            got = events_to_chunk(ev, cfg["model"]["num_bins"], cfg["loader"]["resolution"], self.crop, self.norm_input, self.spike_th)
        else:
            pair = tuple({k: t.to(dev) for k, t in ev.items()} for ev in payload)
            got = event_pairs_to_chunk([pair], cfg["data"]["num_frames"], tuple(cfg["loader"]["resolution"]), self.crop, self.norm_input,
                                       self.spike_th, want_event_mask=em is not None, num_chunks=cfg["data"].get("num_chunks", 2))
            if em is not None:
                got, mask = got
                em.copy_(mask)
                em = None
        x.copy_(got)
        if em is not None:
            # (the loops' own expressions: eval_DSEC_flow_SNN's for the tuple form, eval_MV_flow_SNN's for the dict form)
            em.copy_(got.sum(1).sum(1, keepdim=True).bool() if self.polarity or kind == "voxel" else got.sum(1, keepdim=True).bool())

    # -- the scheme ----------------------------------------------------------------------------------------------------------------
    def _fwd(self, x):
        model = self.model
        if x.shape[0] > 1 and hasattr(model, "forward_replicas") and not model.training:
            return model.forward_replicas(x)["flow"][-1]
        if x.shape[0] == 1:
            return model(x)["flow"][-1]
        return torch.cat([model(x[i:i + 1])["flow"][-1] for i in range(x.shape[0])], 0)      # (no replica form: sample by sample)

    def _slot(self, j, in_shape, hw):
        s = self.slots[j]
        if s is None or s["x"].shape[1:] != in_shape or s["lab"].shape[-2:] != hw:
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
            s = self.slots[j] = {"x": z(self.R, *in_shape), "lab": z(self.R, 2, *hw), "msk": z(self.R, 1, *hw),
                                 "em": z(self.R, 1, *hw) if self.mask_events else None, "fwd": {}, "counts": {}}
        return s

    def _render(self, k, units, s, flow, renders_out):
        """The group's rendered bytes into rows k .. of the caller's buffers, on the current stream: the flows as the loop of the
        samples' form stores them (DSEC forms unmasked, MV forms * mask), the events from the signed voxel where the sample came as
        one ("signed" sums on the scored window) and from the model's input otherwise ("split" sums)."""
        from . import hip
        n, dev = len(units), self.device
        m = None
        if units[0][0] in ("volume", "pairs"):
            m = s["msk"][:n] * s["em"][:n] if self.mask_events else s["msk"][:n]
        if "flow" in renders_out:
            hip.flow_image(flow, m, out=renders_out["flow"][k:k + n])
        if "gtflow" in renders_out:
            hip.flow_image(s["lab"][:n], m, out=renders_out["gtflow"][k:k + n])
        if "submission" in renders_out:
            hip.flow_submission(flow, out=renders_out["submission"][k:k + n])
        if "events" in renders_out:
            counts = torch.empty((n, 2) + tuple(flow.shape[-2:]), dtype=torch.float32, device=dev)
            for i, (kind, payload, _, _) in enumerate(units):
                if kind in ("voxel", "volume"):
                    hip.event_counts(payload.to(dev, torch.float32), self.crop if kind == "voxel" else None, out=counts[i:i + 1])
                else:
                    hip.event_counts(s["x"][i:i + 1], out=counts[i:i + 1])
            hip.event_counts_image(counts, out=renders_out["events"][k:k + n])

    def _issue(self, j, k, units, flows_out, renders_out=None):
        """Group of len(units) samples numbered from k, on stream j."""
        from .spikingjelly_compat import functional
        n, st = len(units), self.streams[j]
        kind, payload, label, _ = units[0]
        oy, ox, h, w = self._window(kind, label)
        st.wait_stream(torch.cuda.current_stream(self.device))              # (what the caller enqueued - samples, the table - comes first)
        with torch.cuda.stream(st):
            s = self._slot(j, self._input_shape(kind, payload, (h, w)), (h, w))
            for i, (kind, payload, label, mask) in enumerate(units):
                s["lab"][i:i + 1].copy_(label[..., oy:oy + h, ox:ox + w], non_blocking=True)
                s["msk"][i:i + 1].copy_(mask[..., oy:oy + h, ox:ox + w], non_blocking=True)
                self._prepare(kind, payload, s["x"][i:i + 1], s["em"][i:i + 1] if self.mask_events else None)
            x = s["x"][:n]
            functional.reset_net(self.model)
            mon = self.monitor
            if mon is not None and n not in s["counts"]:
                # the slot's static count block of this group size: the sequence zeroes it and adds every record's counts into it
                s["counts"][n] = torch.zeros((n, len(mon.names), mon.Tmax), dtype=torch.int64, device=self.device)
            block = s["counts"][n] if mon is not None else None

            def fwd():
                if mon is None:
                    return self._fwd(x)
                block.zero_()
                with mon.into(block):
                    return self._fwd(x)
            if not self.graphs:
                flow = fwd()
            else:
                if n not in s["fwd"]:
                    for _ in range(2):
                        fwd()                                            # (also creates this stream's workspaces and plan caches)
                    torch.cuda.synchronize(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        out = fwd()
                    s["fwd"][n] = [g, out]
                g, flow = s["fwd"][n]
                g.replay()
            if mon is not None:
                mon.take(block, first=self._first + k)                   # (into its table's rows, on this stream: as flows_out below)
            self.metrics.update(flow, s["lab"][:n], s["msk"][:n], s["em"][:n] if self.mask_events else None,
                                self.config["metrics"]["flow_scaling"], row=k)
            if flows_out is not None:
                flows_out[k:k + n].copy_(flow, non_blocking=True)
            if renders_out:
                self._render(k, units, s, flow, renders_out)

    def run(self, samples, flows_out=None, renders_out=None):
        """Evaluate the iterable `samples` (the forms of harness.evaluate, or of harness.evaluate_mv when an item is a dict) and return
        the running-mean metrics dict.  `flows_out` (n, 2, h, w): receives every sample's last flow level, in iteration order.
        `renders_out`: a dict of device tensors with any of "flow", "gtflow", "events" ((n, h, w, 3) uint8 RGB) and "submission"
        ((n, h, w, 3) uint16) that receive every sample's rendered images (hip.flow_image / event_image / flow_submission), filled
        on the group's stream right after the metrics: no file is written and no synchronisation added."""
        from .loss.flow_supervised import FlowMetrics
        unknown = set(renders_out or ()) - {"flow", "gtflow", "events", "submission"}
        if unknown:
            raise ValueError(f"renders_out: unknown keys {sorted(unknown)} (flow, gtflow, events, submission)")
        names, rows = None, 64
        if hasattr(samples, "__len__"):
            rows = max(len(samples), 1)
        self.metrics = FlowMetrics(rows, self.device)
        mon = self.monitor
        if mon is not None:
            # sample k of this run is row first + k of the monitor's table, sized now where the number of samples is known; when it has
            # to grow on the way, the growth (a copy on the current stream) waits for every stream's rows first
            was_on, self._first = mon.enabled, mon.forwards
            mon.enable()
            mon.reserve(self._first + rows, self.device)
        try:
            with torch.no_grad():
                for j, k, units in deal(self._units(samples), self.F, self.R):
                    if names is None:
                        default = ["AEE", "AAE"] if units[0][0] in ("volume", "pairs") else ["AEE"]
                        names = self.config["metrics"].get("name", default)
                    if k + len(units) > self.metrics.table.shape[0]:
                        self.metrics.reserve(max(k + len(units), 2 * self.metrics.table.shape[0]))
                    if mon is not None and self._first + k + len(units) > mon.capacity:
                        for st in self.streams:
                            torch.cuda.current_stream(self.device).wait_stream(st)
                        mon.reserve(self._first + k + len(units), self.device)
                    self._issue(j, k, units, flows_out, renders_out)
        finally:
            if mon is not None and not was_on:
                mon.disable()
        return self.metrics.result(tuple(names or ["AEE"]))


def evaluate_stream(model, samples, config, device="cuda", replicas=10, streams=2, graphs=True, flows_out=None, renders_out=None,
                    monitor=None):
    """harness.evaluate / evaluate_mv at the throughput scheme's rate (StreamEvaluator): same sample forms, same config keys
    (loader.crop / polarity, model.norm_input, data.spike_th / num_chunks, metrics.mask_events / flow_scaling / name), every sample a
    batch-1 evaluation (a loader batch of B yields B of them), one host synchronisation at the end.  `flows_out` (n, 2, h, w) receives
    the last flow level of every sample in iteration order; `renders_out`: StreamEvaluator.run's dict of device buffers for the rendered
    images (`vis.store` itself is refused here: no files under this scheme).  graphs=False issues the launch sequences eagerly.
    `monitor`: a monitor.ReplicaFiringRateMonitor of the model - every sample's firing-rate record goes to its table in iteration order
    (monitor.counts(), .mean(), .to_csv(path)): each stream slot owns a static count block per group size that the (captured) sequence
    zeroes and fills and that is copied into the table on the group's stream, as `flows_out` is; no synchronisation is added."""
    return StreamEvaluator(model, config, device, replicas, streams, graphs, monitor).run(samples, flows_out, renders_out)
