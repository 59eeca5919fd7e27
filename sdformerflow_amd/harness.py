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


def events_to_chunk(events, bins, sensor_size, crop, norm_input, spike_th, rectify_map=None):
    """Raw events -> network input (B, bins, 2, h, w) in one HIP launch sequence (hip.event_voxel): voxel grid with the reference's
    semantics (event_representations.py:248-277), centre crop, polarity split, normalisation and spike threshold as
    prepare_chunk(center_crop(grid)) gives them, bit for bit.  `events`: a dict of device tensors 'x', 'y', 'p' and 't' (or 'ts'), or a
    list of B such dicts (one batch; min-max runs over the whole batch tensor, as prepare_chunk does).  x, y: fp32, or integer sensor
    coordinates with `rectify_map` (H_s, W_s, 2).  norm_input "std" runs prepare_chunk's own code on the un-normalised output."""
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
        for k, a in zip("xytp", (x, y, event_times(t), ev["p"].to(torch.float32))):
            cols[k].append(a.reshape(-1))
        offsets.append(offsets[-1] + cols["t"][-1].numel())
    x, y, t, p = (c[0] if len(c) == 1 else torch.cat(c) for c in (cols[k] for k in "xytp"))
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


def evaluate_mv(model, samples, config, device="cuda"):
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


def evaluate(model, samples, config, device="cuda"):
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
        m = AEE(pred, label, mask, config["metrics"]["flow_scaling"])()
        for b in range(pred.shape[0]):
            it += 1
            tot["AEE"] += float(m[0][b])
            for key, v in zip(("PE1", "PE2", "PE3", "outliers"), m[1:]):
                tot[key] += float(v.reshape(-1)[b] if v.numel() > 1 else v)
    return {k: v / max(it, 1) for k, v in tot.items()}
