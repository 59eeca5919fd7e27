"""The training loops' augmentations (reference DSEC_dataloader/data_augmentation.py; train_flow_parallel_supervised_SNN.py:155-171),
restated twice over one set of parameters:

* calling a transform on `(events, flow, mask)` - events (B, bins, H, W), flow (B, 2, H, W), mask (B, 1, H, W) - does what the
  reference's class does, in plain torch on whatever device the tensors are on, drawing from the same generators in the same order
  (`random.randint` for the crop, row then column; `torch.rand(1).item() <= p` per flip; one `torch.rand(1)` each for the drop's coin
  and its q, then `torch.rand_like(events)`).  This is the composition `hip.augment_chunk` is compared with;
* `Compose.sample(shape)` makes the same draws without touching a tensor and returns them as an `AugmentParams` record - what
  `hip.augment_chunk` (csrc/prepare_chunk.hip) takes.  The drop's uniform field is not drawn there: the kernel has its own Philox
  stream, so after a batch that drops `torch`'s generator stands where the reference's stood BEFORE its `rand_like`.

As in the reference one set of parameters serves the whole batch; the kernel's per-sample arrays are filled with equal values.
The rotation (`RandomRotationFlip`) is not built.  The MDR loader's `DenseSparseAugmentor` is MDR_dataloader.loader_utils'.
"""
import numbers
import random
from dataclasses import dataclass

import torch

ACCEPTED = "Compose([CenterCrop | RandomCrop]?, Random_horizontal_flip / Random_vertical_flip in either order, Random_event_drop?)"


@dataclass
class AugmentParams:
    """One batch's draws: window size (h, w) and origin, the flips, the drop's q (None: the events are kept)."""
    crop: tuple
    origin: tuple
    hflip: bool
    vflip: bool
    drop_q: float = None

    @property
    def flags(self):
        return int(self.hflip) | int(self.vflip) << 1

    def per_sample(self, B):
        """(origins, flips, drop_q) as hip.augment_chunk's per-sample lists: equal entries, one draw per batch."""
        return [self.origin] * B, [self.flags] * B, [self.drop_q] * B


def _size(size):
    return (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(size)


def _even(i, j, keep):
    """`preserve_mosaicing_pattern`: an odd origin moves one pixel on."""
    return (i + i % 2, j + j % 2) if keep else (i, j)


def _window(x, i, j, th, tw):
    events, flow, mask = x
    return events[..., i:i + th, j:j + tw], flow[:, :, i:i + th, j:j + tw], mask[:, :, i:i + th, j:j + tw]


class CenterCrop:
    """The central (th, tw) window of the last two dims; the origin rounds half to even, as Python's round does."""

    def __init__(self, size, preserve_mosaicing_pattern=False):
        self.size = _size(size)
        self.preserve_mosaicing_pattern = preserve_mosaicing_pattern

    def origin(self, h, w):
        th, tw = self.size
        assert th <= h and tw <= w
        return _even(int(round((h - th) / 2.)), int(round((w - tw) / 2.)), self.preserve_mosaicing_pattern)

    def __call__(self, x):
        return _window(x, *self.origin(*x[0].shape[-2:]), *self.size)

    def __repr__(self):
        return f"{type(self).__name__}(size={self.size})"


class RandomCrop(CenterCrop):
    """A (th, tw) window at a uniformly drawn origin: `random.randint` for the row, then for the column; no draw when the window is
    the whole image."""

    def origin(self, h, w):
        th, tw = self.size
        assert th <= h and tw <= w
        if (h, w) == (th, tw):
            return 0, 0
        i = random.randint(0, h - th)
        j = random.randint(0, w - tw)
        return _even(i, j, self.preserve_mosaicing_pattern)


class _Flip:
    dim, component = None, None

    def __init__(self, p=0.5):
        self.p = p

    def draw(self):
        return torch.rand(1).item() <= self.p

    def __call__(self, x):
        events, flow, mask = x
        if self.draw():
            events, flow, mask = events.flip(self.dim), flow.flip(self.dim), mask.float().flip(self.dim)
            flow[:, self.component] *= -1
        return events, flow, mask.bool()

    def __repr__(self):
        return f"{type(self).__name__}(p={self.p})"


class Random_horizontal_flip(_Flip):
    """With probability p: the last dim reversed, the flow's x component negated.  The mask leaves as bool either way."""
    dim, component = -1, 0


class Random_vertical_flip(_Flip):
    """With probability p: the rows reversed, the flow's y component negated.  The mask leaves as bool either way."""
    dim, component = -2, 1


class Random_event_drop:
    """With probability p: events * (u > q), u uniform per cell, q uniform between the two drop rates (fp32, as the reference forms it)."""

    def __init__(self, min_drop_rate=0., max_drop_rate=0.6, p=0.5):
        self.p = p
        self.min_drop_rate = min_drop_rate
        self.max_drop_rate = max_drop_rate

    def draw(self):
        """q as a 1-element fp32 tensor, or None (the coin said keep)."""
        if torch.rand(1).item() <= self.p:
            return (self.min_drop_rate - self.max_drop_rate) * torch.rand(1) + self.max_drop_rate
        return None

    def __call__(self, x, u=None):
        """`u`: the uniform field to use instead of `torch.rand_like(events)` (what hip.augment_chunk takes as `drop_u`)."""
        events, flow, mask = x
        q = self.draw()
        if q is not None:
            if u is None:
                u = torch.rand_like(events)
            events = events * (u > q.to(events.device))
        return events, flow, mask

    def __repr__(self):
        return f"{type(self).__name__}(min_drop_rate={self.min_drop_rate}, max_drop_rate={self.max_drop_rate}, p={self.p})"


class RandomRotationFlip:
    """The reference's rotation by bilinear resampling: not built (its loops keep it commented out)."""

    def __init__(self, degrees, p_hflip=0.5, p_vflip=0.5):
        raise NotImplementedError("RandomRotationFlip (a bilinear rotation of events, flow and mask) is not built - use "
                                  "Random_horizontal_flip and Random_vertical_flip, as the reference's training loops do")


class Compose:
    """The transforms one after the other.  `sample(shape)` needs the chain in the accepted order; calling it does not."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x, drop_u=None):
        for t in self.transforms:
            x = t(x, drop_u) if isinstance(t, Random_event_drop) and drop_u is not None else t(x)
        return x

    def chain(self):
        """(crop or None, [flips in their order], drop or None); ValueError for anything but the accepted order."""
        rest = list(self.transforms)
        crop = rest.pop(0) if rest and isinstance(rest[0], CenterCrop) else None
        drop = rest.pop() if rest and isinstance(rest[-1], Random_event_drop) else None
        kinds = [type(t) for t in rest]
        if any(k not in (Random_horizontal_flip, Random_vertical_flip) for k in kinds) or len(set(kinds)) != len(kinds):
            raise ValueError(f"Compose.sample: the accepted chain is {ACCEPTED}, got {self!r}")
        return crop, rest, drop

    def sample(self, shape):
        """The parameter record of one batch of `shape` (..., H, W), drawn as __call__ draws - the crop's origin, a coin per flip, the
        drop's coin and q - without the drop's uniform field."""
        crop, flips, drop = self.chain()
        H, W = int(shape[-2]), int(shape[-1])
        size, origin = ((H, W), (0, 0)) if crop is None else (tuple(crop.size), crop.origin(H, W))
        on = {type(t): t.draw() for t in flips}
        q = drop.draw() if drop is not None else None
        return AugmentParams(size, origin, on.get(Random_horizontal_flip, False), on.get(Random_vertical_flip, False),
                             None if q is None else float(q.item()))

    def __repr__(self):
        return type(self).__name__ + "(" + "".join(f"\n    {t}" for t in self.transforms) + "\n)"
