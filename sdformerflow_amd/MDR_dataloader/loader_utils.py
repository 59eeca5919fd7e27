"""`EventSequence` and `EventSequenceToVoxelGrid_Pytorch` of the reference (MDR_dataloader/loader_utils.py:344-389, 421-577) by name
and call form, on device tensors, served by the HIP voxeliser (csrc/event_voxel_tb.hip through hip.event_voxel_tb).  The grid has the
bits the reference class produces on the CPU before normalisation, and its normalisation evaluated in float64.  There is no CPU path:
CPU tensors raise SdfError.

`DenseSparseAugmentor` (:244-341), the augmentor of every MDR training item, by name as well:
* called on numpy H x W x C arrays it is the reference's `spatial_transform` in numpy, draw for draw from numpy's global generator,
  with `resize_linear` - cv2.resize(INTER_LINEAR) restated as OpenCV documents and implements it - in cv2's place;
* `sample(shape)` makes the same draws without touching an array and returns them as a `ResizeParams` record - what
  `hip.augment_resize_chunk` (csrc/prepare_chunk.hip, sdf_augment_resize_fwd) takes; `sample_batch(B, shape)` draws per item, as the
  reference's Dataset.__getitem__ does.
The eraser and `photo_aug` are dead code in the reference and are not built; neither is `FlowAugmentor`, which MDR.py reaches only
through an attribute it never sets.  The .npz / .flo / HDF5 readers are out of scope.  No cv2, torchvision or pandas import."""
from dataclasses import dataclass

import numpy
import torch

from .. import hip


def _linear_axis(n_src, n_dst, f):
    """One axis of cv2.resize(INTER_LINEAR): for every destination index the first tap, the second tap and the second tap's weight.
    s = 1 / f in float64; c = float32((d + 0.5) s - 0.5) with the product and the difference in float64; i = floor(c), a = c - i in
    float32; i < 0: i = 0, a = 0; i >= n - 1: i = n - 1, a = 0; the second tap is min(i + 1, n - 1)."""
    s = 1.0 / float(f)
    c = ((numpy.arange(n_dst, dtype=numpy.float64) + 0.5) * s - 0.5).astype(numpy.float32)
    fl = numpy.floor(c)
    i = fl.astype(numpy.int64)
    a = c - fl                                                              # (float32 - float32)
    low, high = i < 0, i >= n_src - 1
    i = numpy.where(low, 0, numpy.where(high, n_src - 1, i))
    a = numpy.where(low | high, numpy.float32(0), a).astype(numpy.float32)
    return i, numpy.minimum(i + 1, n_src - 1), a


def resize_size(shape, fx, fy):
    """(rows, columns) of cv2.resize(img, None, fx=fx, fy=fy) for an image of `shape` (H, W): rint(H fy), rint(W fx), half to even
    (cvRound)."""
    return int(numpy.rint(shape[0] * float(fy))), int(numpy.rint(shape[1] * float(fx)))


def resize_linear(img, fx, fy):
    """cv2.resize(img, None, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) for a float32 image (H, W) or (H, W, C), restated: the
    output size of `resize_size`, the taps and weights of `_linear_axis` per axis, the horizontal pass r = S[i] (1 - a) + S[i + 1] a
    first and the vertical pass on its results, each product and each sum rounded to float32 on its own (no fused multiply-add).  A
    real cv2 build may fuse the vertical pass or take another path, so it can differ in the last bit: this restatement has not been
    compared with one."""
    img = numpy.asarray(img)
    if img.dtype != numpy.float32 or img.ndim not in (2, 3):
        raise ValueError(f"resize_linear: a float32 image (H, W) or (H, W, C), got {img.dtype} {img.shape}")
    H, W = img.shape[:2]
    h, w = resize_size((H, W), fx, fy)
    x0, x1, ax = _linear_axis(W, w, fx)
    y0, y1, ay = _linear_axis(H, h, fy)
    one = numpy.float32(1)
    wide = (slice(None),) * 2 + (None,) * (img.ndim - 2)                    # weights against (rows, columns[, channels])
    ax0, ax1 = (one - ax)[None, :][wide], ax[None, :][wide]
    ay0, ay1 = (one - ay)[:, None][wide], ay[:, None][wide]
    rows = img[:, x0] * ax0 + img[:, x1] * ax1
    return rows[y0] * ay0 + rows[y1] * ay1


@dataclass
class ResizeParams:
    """One item's draws of DenseSparseAugmentor: whether it is rescaled, the scales (float64, after the clip), the resized size
    (rows, columns; the source's when not rescaled), the flips, and the crop origin in the flipped, resized image."""
    resized: bool
    scale_x: float
    scale_y: float
    size: tuple
    hflip: bool
    vflip: bool
    y0: int
    x0: int


def flow_valid(flow):
    """MDR.py:234 on an (H, W, 2) flow: ~isinf(u) & ~isinf(v) & (norm > 0), in the flow's own precision."""
    return numpy.logical_and(numpy.logical_and(~numpy.isinf(flow[:, :, 0]), ~numpy.isinf(flow[:, :, 1])), numpy.linalg.norm(flow, axis=2) > 0)


class DenseSparseAugmentor:
    """Random rescale, stretch, flips and crop of the two event-volume pairs and the flow of an MDR training item."""

    def __init__(self, crop_size, min_scale=-0.2, max_scale=0.5, do_flip=False):
        self.crop_size = crop_size
        self.min_scale = min_scale
        self.max_scale = max_scale
        self.spatial_aug_prob = 0.8
        self.stretch_prob = 0.8
        self.max_stretch = 0.2
        self.do_flip = do_flip
        self.h_flip_prob = 0.5
        self.v_flip_prob = 0.1

    def sample(self, shape):
        """The draws of one call on images of `shape` (H, W), in the reference's order - uniform (scale); rand (stretch) and its two
        uniform; rand (resize); rand per flip; two randint - from numpy's global generator, as a ResizeParams."""
        ht, wd = shape
        rnd = numpy.random
        floor = numpy.maximum((self.crop_size[0] + 8) / float(ht), (self.crop_size[1] + 8) / float(wd))
        scale_x = scale_y = 2 ** rnd.uniform(self.min_scale, self.max_scale)
        if rnd.rand() < self.stretch_prob:
            scale_x *= 2 ** rnd.uniform(-self.max_stretch, self.max_stretch)
            scale_y *= 2 ** rnd.uniform(-self.max_stretch, self.max_stretch)
        scale_x, scale_y = numpy.clip(scale_x, floor, None), numpy.clip(scale_y, floor, None)
        resized = bool(rnd.rand() < self.spatial_aug_prob)
        size = resize_size((ht, wd), scale_x, scale_y) if resized else (int(ht), int(wd))
        hflip = bool(self.do_flip and rnd.rand() < self.h_flip_prob)
        vflip = bool(self.do_flip and rnd.rand() < self.v_flip_prob)
        y0 = rnd.randint(0, size[0] - self.crop_size[0])
        x0 = rnd.randint(0, size[1] - self.crop_size[1])
        return ResizeParams(resized, float(scale_x), float(scale_y), size, hflip, vflip, int(y0), int(x0))

    def sample_batch(self, B, shape):
        """B records in item order: the reference draws in Dataset.__getitem__, once per item."""
        return [self.sample(shape) for _ in range(B)]

    def apply(self, p, img1, img2, dimg1, dimg2, flow):
        """The transform under the draws `p`.  The flow, a float32 array times a Python list, is float64 from its first product on
        (flow * [scale_x, scale_y], then * [-1.0, 1.0] / [1.0, -1.0] under a flip) and stays float32 only when nothing happens to it."""
        imgs = [img1, img2, dimg1, dimg2]
        if p.resized:
            imgs = [resize_linear(a, p.scale_x, p.scale_y) for a in imgs]
            flow = resize_linear(flow, p.scale_x, p.scale_y) * [p.scale_x, p.scale_y]
        if p.hflip:
            imgs = [a[:, ::-1] for a in imgs]
            flow = flow[:, ::-1] * [-1.0, 1.0]
        if p.vflip:
            imgs = [a[::-1, :] for a in imgs]
            flow = flow[::-1, :] * [1.0, -1.0]
        window = (slice(p.y0, p.y0 + self.crop_size[0]), slice(p.x0, p.x0 + self.crop_size[1]))
        return tuple(numpy.ascontiguousarray(a[window]) for a in imgs + [flow])

    def __call__(self, img1, img2, dimg1, dimg2, flow):
        return self.apply(self.sample(img1.shape[:2]), img1, img2, dimg1, dimg2, flow)


class EventSequence(object):
    """`features`: (N, 4) float64 device tensor [ts, x, y, p] (the `dataframe` form is not served: pass None).  As in the reference the
    list is sorted by time when it is not, the stamps are multiplied by `timestamp_multiplier` and made relative to the first - each
    one float64 operation.  Unlike the reference, `features` is not changed in place, and no features means an empty list."""

    def __init__(self, dataframe, params, features=None, timestamp_multiplier=None, convert_to_relative=False):
        if dataframe is not None:
            raise hip.SdfError("EventSequence: pass the events as `features`, an (N, 4) float64 device tensor [ts, x, y, p]")
        if features is None:
            raise hip.SdfError("EventSequence: no features (an empty list is a (0, 4) tensor)")
        if not torch.is_tensor(features) or not features.is_cuda:
            raise hip.SdfError("HIP path needs device tensors (no CPU fallback)")
        if features.dim() != 2 or features.shape[1] != 4 or features.dtype != torch.float64:
            raise hip.SdfError("EventSequence: features is an (N, 4) float64 tensor [ts, x, y, p]")
        self.feature_names = ["ts", "x", "y", "p"]
        self.features = features
        self.image_height = params["height"]
        self.image_width = params["width"]
        if not self.is_sorted():
            self.sort_by_timestamp()
        if timestamp_multiplier is not None:
            self.features = torch.cat((self.features[:, :1] * timestamp_multiplier, self.features[:, 1:]), dim=1)
        if convert_to_relative:
            self.absolute_time_to_relative()

    def get_sequence_only(self):
        return self.features

    def __len__(self):
        return len(self.features)

    def __add__(self, sequence):
        return EventSequence(None, {"height": self.image_height, "width": self.image_width},
                             features=torch.cat([self.features, sequence.features]))

    def is_sorted(self):
        return bool((self.features[:-1, 0] <= self.features[1:, 0]).all())

    def sort_by_timestamp(self):
        if len(self.features) > 0:
            self.features = self.features[torch.sort(self.features[:, 0], stable=True)[1]]

    def absolute_time_to_relative(self):
        """Transforms absolute time to time relative to the first event."""
        if len(self.features) > 0:
            self.features = torch.cat((self.features[:, :1] - self.features[0, 0], self.features[:, 1:]), dim=1)


class EventSequenceToVoxelGrid_Pytorch(object):
    """Voxel grid with bilinear interpolation in the time domain.  `gpu`, `gpu_nr` and `forkserver` are accepted for the call form: the
    grid is built on the device the sequence lives on.  Returns (num_bins, H, W), or (num_bins, 2, H, W) with pol=False."""

    def __init__(self, num_bins, gpu=False, gpu_nr=0, normalize=True, forkserver=True, pol=True):
        self.num_bins = num_bins
        self.normalize = normalize
        self.pol = pol

    def __call__(self, event_sequence):
        f = event_sequence.features
        if not f.is_cuda:
            raise hip.SdfError("HIP path needs device tensors (no CPU fallback)")
        x, y = f[:, 1].to(torch.int32), f[:, 2].to(torch.int32)                 # .long(): truncation toward zero
        return hip.event_voxel_tb(x, y, f[:, 0].contiguous(), f[:, 3].to(torch.float32), self.num_bins,
                                  (event_sequence.image_height, event_sequence.image_width), normalize=self.normalize,
                                  mode="signed" if self.pol else "polarities")[0]
