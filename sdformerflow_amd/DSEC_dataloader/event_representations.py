"""Event representations on the GPU: the reference's `VoxelGrid` (DSEC_dataloader/event_representations.py:241-313) by name and
methods, served by the HIP voxeliser (csrc/event_voxel.hip through hip.event_voxel).  Event dict in - 'x', 'y', 't', 'p' fp32 device
tensors, time-ordered - tensor out, with the bits the reference class produces on the CPU.  There is no CPU path: CPU tensors raise
SdfError.  h5 reading, EventSlicer and count frames are out of scope."""
from .. import hip


def rectify_events(x, y, rectify_map):
    """Integer sensor coordinates -> rectified fp32 (x, y) = rectify_map[y, x] (reference :20-28), as torch indexing on the device.
    (hip.event_voxel takes the integer coordinates and the map directly and fuses this lookup.)"""
    xy = rectify_map[y.long(), x.long()]
    return xy[:, 0], xy[:, 1]


class VoxelGrid:
    def __init__(self, input_size: tuple):
        assert len(input_size) == 3
        self.input_size = tuple(int(v) for v in input_size)
        self.nb_channels = self.input_size[0]

    def _convert(self, events, mode):
        C, H, W = self.input_size
        return hip.event_voxel(events["x"], events["y"], events["t"], events["p"], C, (H, W), mode=mode)[0]

    def convert_CHW(self, events):
        """(C, H, W): bilinear votes of (2p - 1) into the 8 neighbouring cells of (x, y, t_norm)."""
        return self._convert(events, "signed")

    def convert_CHW_polarities(self, events):
        """(C, 2, H, W): unsigned votes of the p == 1 | p == 0 events."""
        return self._convert(events, "polarities")
