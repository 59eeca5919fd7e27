"""hip.augment_chunk (csrc/prepare_chunk.hip, sdf_augment_chunk_fwd) restated in numpy, one fp32 operation per step as the kernel
has them: the gather with its sign rule, the drop, the polarity split, min-max, the threshold, the masks, and Philox4x32-10.
Shared by tests/test_augment_cpu.py (against the reference's transforms, tests/golden/augment.npz) and tests/test_augment_gpu.py
(against the kernel).  Also: the transform chains of the fixture by name."""
import numpy as np

F32 = np.float32
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11) of `counter` (4 words) under `key`
    (2 words): arrays of uint32 values, broadcast against each other; returns the four output words as uint64 arrays below 2^32."""
    c = [np.asarray(w, dtype=np.uint64) & M32 for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & M32 for w in key]
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]          # (32 x 32 bits: no overflow in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & M32, (k[1] + np.uint64(PHILOX_W1)) & M32]
    return c


def philox_uniform(n, seed, offset):
    """The kernel's uniform field for cells 0 .. n-1: key = seed, counter = (i >> 2, offset), word i & 3, u = (word >> 8) 2^-24."""
    i = np.arange(n, dtype=np.uint64)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    blk = i >> np.uint64(2)
    words = philox4x32_10((blk & M32, blk >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((i & np.uint64(3)).astype(np.int64), words)
    return (word >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def gather(voxel, label, valid, crop, origins, flips, drop_q=None, drop_u=None, seed=0, offset=0):
    """Crop, flips and drop: output pixel (y, x) of sample b reads the source at (oy + (vflip ? h-1-y : y), ox + (hflip ? w-1-x : x));
    the flow's x component is negated under a horizontal, its y component under a vertical flip; the mask is valid != 0 as 0 / 1;
    v = v * (u > q) for a sample with q >= 0.  Returns (events (B, bins, h, w), flow (B, 2, h, w) or None, mask (B, 1, h, w) or None)."""
    B, bins, Hs, Ws = voxel.shape
    h, w = crop if crop else (Hs, Ws)
    ev = np.empty((B, bins, h, w), F32)
    fl = None if label is None else np.empty((B, 2, h, w), F32)
    mk = None if valid is None else np.empty((B, 1, h, w), F32)
    u_all = None
    for b in range(B):
        (oy, ox), f = origins[b], flips[b]
        assert 0 <= oy <= Hs - h and 0 <= ox <= Ws - w and 0 <= f <= 3
        ys = oy + (np.arange(h)[::-1] if f & 2 else np.arange(h))
        xs = ox + (np.arange(w)[::-1] if f & 1 else np.arange(w))
        ev[b] = voxel[b][:, ys][:, :, xs]
        if fl is not None:
            fl[b] = label[b][:, ys][:, :, xs]
            if f & 1:
                fl[b, 0] = -fl[b, 0]
            if f & 2:
                fl[b, 1] = -fl[b, 1]
        if mk is not None:
            mk[b, 0] = (valid.reshape(B, Hs, Ws)[b][ys][:, xs] != 0).astype(F32)
        q = None if drop_q is None else drop_q[b]
        if q is not None and not q < 0:
            if drop_u is not None:
                u = drop_u[b]
            else:
                if u_all is None:
                    u_all = philox_uniform(B * bins * h * w, seed, offset).reshape(B, bins, h, w)
                u = u_all[b]
            ev[b] = ev[b] * (u > F32(q)).astype(F32)
    return ev, fl, mk


def prepare(events, norm=None, per_sample=False, spike_th=None):
    """The loop's preparation of (B, bins, h, w) signed events: relu(v) | relu(-v) on dim 2, (v - lo) / (hi - lo) on the non-zeros -
    lo / hi their min / max over the batch tensor or each sample - when there is one and lo != hi, the threshold (> th: 1, < th: 0),
    and the event mask (B, 1, h, w): 1 where a pixel has a non-zero element.  Returns (out (B, bins, 2, h, w), event mask)."""
    zero = F32(0)
    out = np.stack((np.where(events > 0, events, zero), np.where(-events > 0, -events, zero)), axis=2).astype(F32)
    if norm == "minmax":
        for grp in ([slice(b, b + 1) for b in range(out.shape[0])] if per_sample else [slice(None)]):
            blk = out[grp]
            nz = blk != 0
            if nz.any():
                lo, hi = blk[nz].min(), blk[nz].max()
                if lo != hi:
                    blk[nz] = (blk[nz] - lo) / (hi - lo)
                    out[grp] = blk
    else:
        assert norm is None
    if spike_th is not None:
        th = F32(spike_th)
        out = np.where(out > th, F32(1), np.where(out < th, zero, out)).astype(F32)
    return out, (out != 0).any(axis=(1, 2))[:, None].astype(F32)


def augment(voxel, label, valid, crop, origins, flips, drop_q=None, drop_u=None, seed=0, offset=0, norm=None, per_sample=False,
            spike_th=None, mask_events=False):
    """The whole of sdf_augment_chunk_fwd: {"out", "label", "mask", "event_mask"}."""
    ev, fl, mk = gather(voxel, label, valid, crop, origins, flips, drop_q, drop_u, seed, offset)
    out, em = prepare(ev, norm, per_sample, spike_th)
    if mask_events:
        mk = mk * em
    return {"out": out, "label": fl, "mask": mk, "event_mask": em}


# ------------------------------------------------------------------------------------------------ the fixture's chains
CROP = (8, 10)
SHAPE = (2, 3, 11, 13)


def chain_names():
    """Every chain of the accepted form as a name: an optional crop, the flips in either order, an optional drop."""
    crops = ("", "RandomCrop", "CenterCrop", "RandomCropEven", "CenterCropEven")
    flips = ("", "H", "V", "H,V", "V,H")
    names = []
    for c in crops:
        for f in flips:
            if c.endswith("Even") and f != "H,V":                  # preserve_mosaicing_pattern: one flip order is enough
                continue
            for d in ("", "Drop"):
                names.append(",".join(p for p in (c, f, d) if p))
    return names


def build_chain(mod, name):
    """`name` as a Compose of the classes of `mod` (the reference's module, or sdformerflow_amd.DSEC_dataloader.data_augmentation)."""
    parts = {"RandomCrop": lambda: mod.RandomCrop(CROP), "CenterCrop": lambda: mod.CenterCrop(CROP),
             "RandomCropEven": lambda: mod.RandomCrop(CROP, preserve_mosaicing_pattern=True),
             "CenterCropEven": lambda: mod.CenterCrop(CROP, preserve_mosaicing_pattern=True),
             "H": lambda: mod.Random_horizontal_flip(0.5), "V": lambda: mod.Random_vertical_flip(0.5),
             "Drop": lambda: mod.Random_event_drop(0., 0.6, 0.5)}
    return mod.Compose([parts[p]() for p in name.split(",") if p])
