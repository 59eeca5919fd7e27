"""Evaluation metrics of the reference (loss/flow_supervised.py): AEE (+ PE1/2/3, outliers) :108-149, AAE :152-175."""
import math

import torch


class AEE(torch.nn.Module):
    """Average end-point error over valid pixels; call the instance to get (AEE[B], PE1, PE2, PE3, outliers)."""

    def __init__(self, pred, label, mask, flow_scaling=128):
        super().__init__()
        self.flow, self.label, self.mask, self.flow_scaling = pred, label, mask, flow_scaling

    def forward(self):
        flow = self.flow * self.flow_scaling
        B = flow.shape[0]
        mask = self.mask.reshape(B, -1)
        err = (flow - self.label).pow(2).sum(1).sqrt().view(B, -1) * mask
        mag = flow.pow(2).sum(1).sqrt().view(B, -1) * mask
        n = mask.sum(dim=1)
        aee = err.sum(dim=1) / (n + 1e-9)
        outliers = ((err > 3.0) * (err > 0.05 * mag)).sum() / (n + 1e-9)
        pe = [(err > th).sum() / (n + 1e-9) for th in (1.0, 2.0, 3.0)]
        return aee, pe[0], pe[1], pe[2], outliers


class AAE(torch.nn.Module):
    """Average angular error in degrees; returns a 1-tuple like the reference (:175)."""

    def __init__(self, pred, label, mask, flow_scaling=128):
        super().__init__()
        self.flow, self.label, self.mask, self.flow_scaling = pred, label, mask, flow_scaling

    def forward(self):
        flow = self.flow * self.flow_scaling
        fm = flow.pow(2).sum(1).sqrt() * self.mask
        gm = self.label.pow(2).sum(1).sqrt() * self.mask
        dot = flow[:, 0] * self.label[:, 0] + flow[:, 1] * self.label[:, 1]
        cos = torch.clamp((dot + 1e-7) / (fm * gm + 1e-7), min=-1.0 + 1e-7, max=1.0 - 1e-7)
        return (torch.sum(torch.acos(cos) * self.mask) / torch.sum(self.mask) * 180 / math.pi,)


class FlowMetrics:
    """The same metrics accumulated on the device: owns a (rows, 8) float64 table of per-sample sums (hip.FLOW_METRICS_FIELDS);
    `update` enqueues hip.flow_metrics for the next rows on the current stream and reads nothing back; `result` synchronises once and
    forms, in fp64 on the host, the dict harness.evaluate / evaluate_mv return.  Every sample is a batch-1 evaluation of the classes
    above (their batch-coupled forms at B > 1 are not reproduced)."""

    def __init__(self, rows, device="cuda"):
        self.table = torch.zeros((int(rows), 8), dtype=torch.float64, device=device)
        self.n = 0

    def update(self, pred, label, mask, event_mask=None, flow_scaling=128, row=None):
        """pred, label (B, 2, H, W); mask, event_mask (B, H, W) or (B, 1, H, W): B more samples, at rows `row` .. (default: the next)."""
        from .. import hip
        row = self.n if row is None else int(row)
        hip.flow_metrics(pred, label, mask, event_mask, flow_scaling, table=self.table, row=row)
        self.n = max(self.n, row + pred.shape[0])
        return self

    def reserve(self, rows):
        """Room for `rows` samples: a larger table takes over the records so far (synchronises when it has to grow)."""
        if rows > self.table.shape[0]:
            if self.table.is_cuda:
                torch.cuda.synchronize(self.table.device)
            table = torch.zeros((int(rows), 8), dtype=torch.float64, device=self.table.device)
            table[:self.table.shape[0]] = self.table
            self.table = table
        return self

    def counts(self):
        """The raw table of the samples so far (on the device; reading it synchronises)."""
        return self.table[:self.n]

    def result(self, names=("AEE", "AAE")):
        """Running means over the samples: AEE = sum_err / (n + 1e-9) with PE1-3 and outliers = count / (n + 1e-9), and
        AAE = sum_ang / n * 180 / pi (NaN for a sample without a valid pixel, as the class gives it)."""
        if self.table.is_cuda:
            torch.cuda.synchronize(self.table.device)
        rows = self.table[:self.n].cpu().tolist()
        if any(n not in ("AEE", "AAE") for n in names):
            raise ValueError(f"FlowMetrics serves AEE and AAE, not {list(names)}")
        tot = {k: 0.0 for n in names for k in ((n, "PE1", "PE2", "PE3", "outliers") if n == "AEE" else (n,))}
        for n_valid, sum_err, pe1, pe2, pe3, outl, sum_ang, _ in rows:
            if "AEE" in tot:
                for key, v in zip(("AEE", "PE1", "PE2", "PE3", "outliers"), (sum_err, pe1, pe2, pe3, outl)):
                    tot[key] += v / (n_valid + 1e-9)
            if "AAE" in tot:
                tot["AAE"] += sum_ang / n_valid * 180 / math.pi if n_valid else math.nan
        return {k: v / max(len(rows), 1) for k, v in tot.items()}
