"""Stored results in the reference's shape (utils/visualization.py Visualization_DSEC, `vis.store`): the event image, the estimated and
the ground-truth flow of every evaluated sample as 8-bit PNGs, and the estimated flow in the DSEC benchmark's 16-bit encoding.

Everything is rendered on the GPU (hip.flow_image / flow_submission / event_counts_image, csrc/flow_render.hip) from device tensors; what
crosses to the host is one copy of the finished bytes per image, and the files are written by utils/png.py.  Not built: the live cv2
window (`update`), the frames / `*_window` images (the reference's loops pass None for them; the image of warped events is written by
the loops themselves with fwl=True, harness.evaluate) and the gray / blue_red schemes."""
import os

import numpy as np

from .png import write_png


class Visualization_DSEC:
    """Visualization_DSEC(config, eval_id, path_results): files go to <path_results>/results/eval_<eval_id>/<sequence>/
    {events, flow, gtflow}/%09d.png and .../flow_test/<sequence>/%06d.png, the reference's tree."""

    def __init__(self, kwargs, eval_id=-1, path_results=None):
        self.img_idx = 0
        self.px = (kwargs.get("vis") or {}).get("px")
        self.color_scheme = "green_red"
        self.store_dir = None
        self.store_file = None
        if eval_id >= 0 and path_results is not None:
            self.store_dir = os.path.join(path_results, "results", f"eval_{eval_id}")
            os.makedirs(self.store_dir, exist_ok=True)

    def update(self, events, gtflow, mask, flow, frames=None, events_window=None, masked_window_flow=None, iwe_window=None):
        raise NotImplementedError("the live cv2 window (vis.enabled) is not built: store() writes the same images as files")

    def store(self, events, gtflow, mask, flow, sequence, flow_test=None, frames=None, events_window=None, masked_window_flow=None,
              iwe_window=None, ts=None, idx=None):
        """One file per sample and image.  events: (B, 2, h, w) fp32 per-polarity event sums (the loops' `chunk_vis`); gtflow, flow,
        flow_test: (B, 2, h, w) fp32 or None; all device tensors.  `mask` is accepted and unused, as in the reference (the loops pass
        flows that are already masked where they want them masked).  `idx`: the number of the batch's first file (default: the
        running count, which restarts with every new sequence); it advances by one per sample.  `ts`: a line for timestamps.txt."""
        from .. import hip
        if self.store_dir is None:
            raise ValueError("Visualization_DSEC.store: no store directory - construct with eval_id >= 0 and path_results")
        if not (frames is None and events_window is None and masked_window_flow is None and iwe_window is None):
            raise ValueError("Visualization_DSEC.store: frames / events_window / masked_window_flow / iwe_window are not built; pass None")
        path_to = os.path.join(self.store_dir, sequence)
        if not os.path.exists(path_to):                                 # a new sequence
            for sub in ("events", "flow", "gtflow"):
                os.makedirs(os.path.join(path_to, sub))
            if self.store_file is not None:
                self.store_file.close()
                self.store_file = None
            self.img_idx = 0
        if idx is not None:
            self.img_idx = int(idx)
        images = {"events": hip.event_counts_image(events.detach())}
        if flow is not None:
            images["flow"] = hip.flow_image(flow.detach())
        if gtflow is not None:
            images["gtflow"] = hip.flow_image(gtflow.detach())
        host = {k: v.cpu().numpy() for k, v in images.items()}
        sub16 = None
        if flow_test is not None:
            sub16 = hip.flow_submission(flow_test.detach()).cpu().numpy()
            os.makedirs(os.path.join(self.store_dir, "flow_test", sequence), exist_ok=True)
        for b in range(events.shape[0]):
            for k, v in host.items():
                write_png(os.path.join(path_to, k, "%09d.png" % self.img_idx), v[b])
            if sub16 is not None:
                write_png(os.path.join(self.store_dir, "flow_test", sequence, "%06d.png" % self.img_idx), sub16[b])
            self.img_idx += 1
        if ts is not None:
            if self.store_file is None:
                self.store_file = open(os.path.join(path_to, "timestamps.txt"), "a")
            self.store_file.write(str(ts) + "\n")
            self.store_file.flush()

    @staticmethod
    def flow_to_image(flow_x, flow_y):
        """(H, W) device tensors -> (H, W, 3) u8 device tensor, the colour-wheel image of one flow field."""
        import torch
        from .. import hip
        return hip.flow_image(torch.stack((flow_x, flow_y), 0).unsqueeze(0).float())[0]

    @staticmethod
    def events_to_image(event_cnt, color_scheme="green_red"):
        """(H, W, 2) device tensor of per-polarity counts (the reference's layout) -> the reference's float image (H, W, 3) =
        (0, pos', neg') in [0, 1] as a device tensor: the stored bytes / 255, channels in the reference's order."""
        from .. import hip
        if color_scheme != "green_red":
            raise NotImplementedError(f"events_to_image: the {color_scheme} scheme is not built, only green_red")
        rgb = hip.event_counts_image(event_cnt.permute(2, 0, 1).unsqueeze(0).float().contiguous())[0]
        return rgb.flip(-1).float() / 255.0


def read_submission(path):
    """A flow_test file back as (2, H, W) float64 flow in pixels, and the third channel: the inverse of the benchmark's encoding."""
    from .png import read_png
    img = read_png(path)
    return (img[..., :2].astype(np.float64).transpose(2, 0, 1) - 2 ** 15) / 128.0, img[..., 2]
