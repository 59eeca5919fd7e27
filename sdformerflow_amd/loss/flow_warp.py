"""Flow quality without ground truth: the Flow Warp Loss (Stoffregen et al. 2020, "Reducing the Sim-to-Real Gap for Event Cameras") of
an estimated flow on the raw events it was estimated from.  The events are moved along the flow to the end of their window and
accumulated (hip.event_iwe, nearest mode: integer counts); FWL = var(warped image) / var(unwarped image) over the window's pixels,
above 1 when the flow sharpens the events.  The reference has no counterpart (its visualiser's `iwe` slots stay None); the definition
is csrc/event_iwe.hip's header and DESIGN.md section 5.  No backward pass: this is a metric, not a training loss."""
import math

import torch


def _variance(table, n):
    """Unbiased variance over n pixels from the rows {sum, sum of squares, ...} of hip.iwe_stats, in fp64: (s2 - s1 * s1 / n) / (n - 1)."""
    s1, s2 = table[..., 0], table[..., 1]
    # (device tensors as divisors: torch turns a division by a host scalar into a multiplication by its rounded reciprocal)
    n, n1 = (torch.full_like(s1, float(v)) for v in (n, n - 1))
    return (s2 - s1 * s1 / n) / n1


def _stats_pair(pred, events, sensor_size, crop, flow_scaling, window, tables, row, check, **kw):
    """The statistics of the nearest image warped by the flow and of the unwarped one (scale 0) into rows `row` .. of the two tables."""
    from .. import harness, hip
    for table, scale in zip(tables, (flow_scaling, 0.0)):
        iwe = harness.warp_events(events, pred, sensor_size, crop, scale, window=window, mode="nearest", check=check, **kw)
        hip.iwe_stats(iwe, table=table, row=row)
    return pred.shape[-2] * pred.shape[-1]


class FWL(torch.nn.Module):
    """FWL(pred, events, sensor_size, crop, flow_scaling, window=(0, 1))() -> (fwl (B,) float64 on the device,), in the shape of the
    metric classes of loss/flow_supervised.py.  pred (B, 2, h, w): the flow on the window `crop` (h, w) of `sensor_size` (None: the
    whole sensor), in units of 1 / flow_scaling pixels over the events' window; events: a dict of device tensors 'x', 'y', 'p' and 't'
    (or 'ts'), or a list of B of them (harness.warp_events' forms; `crop_origin`, `rectify_map` as it takes them).  `window` (a, b):
    only the events of that part of the normalised time.  A sample whose unwarped image has no variance gives NaN."""

    def __init__(self, pred, events, sensor_size, crop, flow_scaling=128, window=(0.0, 1.0), **kw):
        super().__init__()
        self.flow, self.events, self.sensor_size, self.crop = pred, events, sensor_size, crop
        self.flow_scaling, self.window, self.kw = flow_scaling, window, kw

    def forward(self):
        B = self.flow.shape[0]
        tables = [torch.zeros((B, 4), dtype=torch.float64, device=self.flow.device) for _ in range(2)]
        n = _stats_pair(self.flow.detach(), self.events, self.sensor_size, self.crop, self.flow_scaling, self.window, tables, 0, True, **self.kw)
        vs, vz = _variance(tables[0], n), _variance(tables[1], n)
        return (torch.where(vz != 0, vs / vz, torch.full_like(vz, math.nan)),)


class FlowWarpMetrics:
    """FWL accumulated on the device, beside loss.flow_supervised.FlowMetrics: owns two (rows, 4) float64 tables of per-sample
    statistics (hip.IWE_STATS_FIELDS) - of the warped and of the unwarped image; `update` enqueues the warps and hip.iwe_stats for the
    next rows on the current stream and reads nothing back (so a list whose times are all equal is not refused: it adds nothing and
    its FWL is NaN); `result` synchronises once and forms, in fp64, {"FWL": mean over the samples, "FWL_samples": [...]}."""

    def __init__(self, rows, device="cuda"):
        self.tables = [torch.zeros((int(rows), 4), dtype=torch.float64, device=device) for _ in range(2)]
        self.pixels = {}                                                 # row -> pixels of its window
        self.n = 0

    def reserve(self, rows):
        """Room for `rows` samples (synchronises when the tables have to grow)."""
        if rows > self.tables[0].shape[0]:
            dev = self.tables[0].device
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            grown = [torch.zeros((int(rows), 4), dtype=torch.float64, device=dev) for _ in range(2)]
            for g, t in zip(grown, self.tables):
                g[:t.shape[0]] = t
            self.tables = grown
        return self

    def update(self, pred, events, sensor_size, crop, flow_scaling=128, window=(0.0, 1.0), row=None, **kw):
        """pred (B, 2, h, w) and its B event lists (FWL's forms): B more samples, at rows `row` .. (default: the next)."""
        row = self.n if row is None else int(row)
        B = pred.shape[0]
        if row + B > self.tables[0].shape[0]:
            self.reserve(max(row + B, 2 * self.tables[0].shape[0]))
        n = _stats_pair(pred.detach(), events, sensor_size, crop, flow_scaling, window, self.tables, row, False, **kw)
        for b in range(B):
            self.pixels[row + b] = n
        self.n = max(self.n, row + B)
        return self

    def counts(self):
        """The raw tables of the samples so far, (warped, unwarped), on the device (reading them synchronises)."""
        return self.tables[0][:self.n], self.tables[1][:self.n]

    def result(self):
        dev = self.tables[0].device
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        warped, unwarped = (t[:self.n].cpu().tolist() for t in self.tables)
        samples = []
        for k, (s, z) in enumerate(zip(warped, unwarped)):
            n = self.pixels.get(k)
            if n is None or n < 2:
                samples.append(math.nan)
                continue
            vs, vz = ((r[1] - r[0] * r[0] / n) / (n - 1) for r in (s, z))
            samples.append(vs / vz if vz != 0 else math.nan)
        return {"FWL": sum(samples) / len(samples) if samples else math.nan, "FWL_samples": samples}
