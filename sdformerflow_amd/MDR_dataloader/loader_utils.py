"""`EventSequence` and `EventSequenceToVoxelGrid_Pytorch` of the reference (MDR_dataloader/loader_utils.py:344-389, 421-577) by name
and call form, on device tensors, served by the HIP voxeliser (csrc/event_voxel_tb.hip through hip.event_voxel_tb).  The grid has the
bits the reference class produces on the CPU before normalisation, and its normalisation evaluated in float64.  There is no CPU path:
CPU tensors raise SdfError.  The .npz / .flo / HDF5 readers and the augmentors are out of scope."""
import torch

from .. import hip


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
