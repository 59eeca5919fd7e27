"""hip.flow_metrics (csrc/flow_metrics.hip) against the package's torch formulas of the reference's AEE / AAE classes, per sample.

What is exact: the four counts and n_valid (integers; every per-pixel operation is one IEEE fp32 operation in both, so the formulas give
the same flags on the GPU and on the CPU), reproducibility, and independence of the batching.  sum_err is the fp64 sum of the same
fp32 values torch sums: n_pixels 2^-53 relative.  sum_ang goes through acosf, which is not correctly rounded: the yardstick is a
float64 acos of the same fp32 cosines, the bound 4 x the error torch's own fp32 acos (on the same device) shows against it - the margin
convention of the time-bilinear front end - plus the fp64 summation allowance of sum_err.  Measured on the
MI355X: torch's error is at most 1.26e-6 on a sum of 459 rad (32 x 64 pixels; 4.3e-7 on 428 rad at 37 x 53), and the kernel's is the
same figure in every case here - its acosf is the device function torch calls."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu
# B = 3 at a pixel count that is no multiple of a wave (64) or of a workgroup's tile (1024 pixels); one row shorter than two waves;
# exactly one and exactly two workgroups per sample
SHAPES = [(3, 37, 53), (1, 1, 65), (1, 32, 32), (1, 32, 64)]
_CASES = {}


def make_case(B, H, W, scaling):
    """pred, label, valid, event mask on the CPU: errors spread over 0 .. 6 px around the thresholds; sample 1 of a batch has no valid
    pixel; the first pixels of sample 0 are the threshold edges (see test_threshold_edges)."""
    g = np.random.Generator(np.random.PCG64(1000 * B + H * W))
    label = g.normal(0.0, 5.0, (B, 2, H, W)).astype(np.float32)
    flow = (label + g.normal(0.0, 1.6, (B, 2, H, W))).astype(np.float32)
    valid = (g.random((B, H, W)) < 0.7).astype(np.float32)
    emask = (g.random((B, H, W)) < 0.6).astype(np.float32)
    if B > 1:
        valid[1] = 0.0
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    edges = [(1.0, 0.0), (up(1.0), 0.0), (2.0, 0.0), (up(2.0), 0.0), (3.0, 0.0), (up(3.0), 0.0),
             (100.0, 96.5), (60.0, 56.5)]                          # e = 3.5 at 0.05f mag = 5.0000001 | 3.0000002: not an outlier | one
    if H * W >= 64:
        for i, (fx, lx) in enumerate(edges):
            flow.reshape(B, 2, -1)[0, :, i] = (fx, 0.0)
            label.reshape(B, 2, -1)[0, :, i] = (lx, 0.0)
            valid.reshape(B, -1)[0, i] = emask.reshape(B, -1)[0, i] = 1.0
    pred = (flow / np.float32(scaling)).astype(np.float32)             # (scaling is a power of two: pred * scaling == flow)
    return tuple(torch.from_numpy(a) for a in (pred, label, valid, emask))


def formulas(pred, label, valid, emask, scaling):
    """The classes' per-pixel fp32 expressions (loss/flow_supervised.py AEE.forward, AAE.forward) on ONE sample (1, ...), on the
    tensors' device: e, mag, m, cos as (H W,) fp32."""
    flow = pred * scaling
    mask = valid.unsqueeze(1)
    if emask is not None:
        mask = mask * emask.unsqueeze(1)
    m = mask.reshape(1, -1)
    err = (flow - label).pow(2).sum(1).sqrt().view(1, -1) * m
    mag = flow.pow(2).sum(1).sqrt().view(1, -1) * m
    fm = flow.pow(2).sum(1).sqrt() * mask
    gm = label.pow(2).sum(1).sqrt() * mask
    dot = flow[:, 0] * label[:, 0] + flow[:, 1] * label[:, 1]
    cos = torch.clamp((dot + 1e-7) / (fm * gm + 1e-7), min=-1.0 + 1e-7, max=1.0 - 1e-7)
    return err[0], mag[0], m[0], cos.reshape(-1)


def record(err, mag, m):
    """{n_valid, n_pe1, n_pe2, n_pe3, n_outlier} as integers, as the class counts them."""
    return [int(m.double().sum()), int((err > 1.0).sum()), int((err > 2.0).sum()), int((err > 3.0).sum()),
            int(((err > 3.0) * (err > 0.05 * mag)).sum())]


def case(B, H, W, scaling, use_em):
    """Inputs, the kernel's table, and the torch references - computed once, shared, never changed."""
    key = (B, H, W, scaling, use_em)
    if key not in _CASES:
        from sdformerflow_amd import hip
        cpu = make_case(B, H, W, scaling)
        dev = tuple(t.to(DEV) for t in cpu)
        em = dev[3] if use_em else None
        table = hip.flow_metrics(dev[0], dev[1], dev[2], em, scaling)
        refs = []
        for b in range(B):
            one = lambda ts: (ts[0][b:b + 1], ts[1][b:b + 1], ts[2][b:b + 1], ts[3][b:b + 1] if use_em else None)
            e_g, mag_g, m_g, cos_g = formulas(*one(dev), scaling)
            e_c, mag_c, m_c, _ = formulas(*one(cpu), scaling)
            yard = (torch.acos(cos_g.double()) * m_g.double()).sum().item()
            torch_ang = (torch.acos(cos_g) * m_g).double().sum().item()
            refs.append({"gpu": record(e_g, mag_g, m_g), "cpu": record(e_c, mag_c, m_c), "sum_err": e_g.double().sum().item(),
                         "yard": yard, "torch_ang": torch_ang, "e": e_g})
        _CASES[key] = (dev, em, table, table.cpu().numpy().copy(), refs)
    return _CASES[key]


@pytest.mark.parametrize("use_em", [False, True])
@pytest.mark.parametrize("scaling", [1, 128])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_records_against_the_torch_formulas(B, H, W, scaling, use_em):
    from sdformerflow_amd import hip
    from sdformerflow_amd.loss.flow_supervised import AAE, AEE
    dev, em, table, got, refs = case(B, H, W, scaling, use_em)
    assert got.shape == (B, 8) and got.dtype == np.float64
    px = H * W
    for b, ref in enumerate(refs):
        n, s_err, pe1, pe2, pe3, outl, s_ang, npx = got[b]
        ints = [n, pe1, pe2, pe3, outl]
        assert all(float(v).is_integer() for v in ints) and npx == px
        assert [int(v) for v in ints] == ref["gpu"] == ref["cpu"], (b, ints, ref["gpu"], ref["cpu"])
        assert abs(s_err - ref["sum_err"]) <= px * 2.0 ** -53 * abs(ref["sum_err"]), (b, s_err, ref["sum_err"])
        torch_err = abs(ref["torch_ang"] - ref["yard"])
        kernel_err = abs(s_ang - ref["yard"])
        print("B %d %dx%d scaling %d em %d sample %d: sum_ang error vs float64 acos: kernel %.3e, torch fp32 acos %.3e (sum %.6g)"
              % (B, H, W, scaling, use_em, b, kernel_err, torch_err, ref["yard"]))
        assert kernel_err <= 4.0 * torch_err + px * 2.0 ** -53 * abs(ref["yard"]), (b, kernel_err, torch_err)
        # and the classes themselves on this sample (the tolerance tests/test_harness.py gives the torch class)
        mask = (dev[2][b:b + 1] * em[b:b + 1] if em is not None else dev[2][b:b + 1]).unsqueeze(1)
        cls = [float(v.reshape(-1)[0]) for v in AEE(dev[0][b:b + 1], dev[1][b:b + 1], mask, scaling)()]
        mine = [v / (n + 1e-9) for v in (s_err, pe1, pe2, pe3, outl)]
        assert np.allclose(mine, cls, rtol=1e-6, atol=1e-9), (b, mine, cls)
        if n:                                                          # (the class sums <= 2048 fp32 terms: ~ log2(N) 2^-24 = 7e-7, and its acos)
            aae = float(AAE(dev[0][b:b + 1], dev[1][b:b + 1], mask, scaling)()[0])
            assert abs(s_ang / n * 180 / np.pi - aae) <= 1e-5 * aae, (b, s_ang / n * 180 / np.pi, aae)
    # a second call gives the same bits; so do B calls of one sample each
    again = hip.flow_metrics(dev[0], dev[1], dev[2], em, scaling).cpu().numpy()
    assert np.array_equal(again.view(np.int64), got.view(np.int64))
    for b in range(B if B > 1 else 0):
        one = hip.flow_metrics(dev[0][b:b + 1], dev[1][b:b + 1], dev[2][b:b + 1], em[b:b + 1] if em is not None else None, scaling)
        assert np.array_equal(one.cpu().numpy().view(np.int64), got[b:b + 1].view(np.int64)), b


def test_threshold_edges():
    """e exactly 1.0, 2.0, 3.0 is not counted, the next float above is; at e = 3.5 one pixel lies on each side of e > 0.05f * mag."""
    dev, em, table, got, refs = case(3, 37, 53, 1, False)
    e = refs[0]["e"][:8].cpu().numpy()
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    assert list(e[:6]) == [1.0, up(1.0), 2.0, up(2.0), 3.0, up(3.0)] and e[6] == 3.5 and e[7] == 3.5
    from sdformerflow_amd import hip
    first8 = lambda t, c: t[0].reshape(c, -1)[:, :8].reshape(1, c, 1, 8).contiguous()
    sub = hip.flow_metrics(first8(dev[0], 2), first8(dev[1], 2), first8(dev[2], 1), None, 1).cpu().numpy()[0]
    # {n_valid, sum_err, n_pe1, n_pe2, n_pe3, n_outlier, sum_ang, n_pixels}: pe1 counts up(1), 2, up(2), 3, up(3), 3.5, 3.5 ...
    assert sub[0] == 8 and sub[2] == 7 and sub[3] == 5 and sub[4] == 3 and sub[5] == 2 and sub[7] == 8
    # (up(3) is an outlier too: 0.05f * mag = 0.15; of the two pixels at 3.5 only the one with mag 60 is)
    assert sub[1] == float(np.sum(e.astype(np.float64)))


def test_a_sample_without_a_valid_pixel_gives_zero_not_nan():
    from sdformerflow_amd.loss.flow_supervised import FlowMetrics
    dev, em, table, got, refs = case(3, 37, 53, 128, True)
    assert not got[1, :7].any() and got[1, 7] == 37 * 53 and np.isfinite(got).all()
    m = FlowMetrics(1, DEV).update(dev[0][1:2], dev[1][1:2], dev[2][1:2], em[1:2], 128)
    assert m.result(("AEE",)) == {"AEE": 0.0, "PE1": 0.0, "PE2": 0.0, "PE3": 0.0, "outliers": 0.0}


def test_rows_outside_the_call_are_left_untouched():
    from sdformerflow_amd import hip
    dev, em, table, got, refs = case(3, 37, 53, 1, True)
    big = torch.full((7, 8), -12345.5, dtype=torch.float64, device=DEV)
    out = hip.flow_metrics(dev[0], dev[1], dev[2], em, 1, table=big, row=2)
    assert out is big
    host = big.cpu().numpy()
    assert (host[:2] == -12345.5).all() and (host[5:] == -12345.5).all()
    assert np.array_equal(host[2:5].view(np.int64), got.view(np.int64))
    with pytest.raises(hip.SdfError):
        hip.flow_metrics(dev[0], dev[1], dev[2], em, 1, table=big, row=5)          # rows 5 .. 7 of 7
    assert np.array_equal(big.cpu().numpy(), host)


def test_flow_metrics_class_accumulates_without_reading_back():
    from sdformerflow_amd.loss.flow_supervised import FlowMetrics
    dev, em, table, got, refs = case(3, 37, 53, 1, False)
    m = FlowMetrics(5, DEV)
    m.update(dev[0][:2], dev[1][:2], dev[2][:2], None, 1).update(dev[0][2:], dev[1][2:], dev[2][2:].unsqueeze(1), None, 1)
    assert m.n == 3 and np.array_equal(m.counts().cpu().numpy().view(np.int64), got.view(np.int64))
    res = m.result(("AEE",))
    want = np.mean([got[b, 1] / (got[b, 0] + 1e-9) for b in range(3)])
    assert abs(res["AEE"] - want) <= 1e-15 * want and set(res) == {"AEE", "PE1", "PE2", "PE3", "outliers"}


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_fixture_pin(kind):
    """The reference's own flow map and AEE tuple (tests/golden/end_to_end.npz), at the tolerance tests/test_harness.py gives the
    torch class."""
    from sdformerflow_amd import hip
    from sdformerflow_amd.synthetic import synth_label
    G = np.load(os.path.join(ROOT, "tests", "golden", "end_to_end.npz"))
    flow = torch.from_numpy(G[f"{kind}_flow3"]).repeat_interleave(2, -1).repeat_interleave(2, -2)
    label, mask = synth_label(1, 288, 384)
    t = hip.flow_metrics(flow.to(DEV), label.to(DEV), mask.to(DEV), None, 1).cpu().numpy()[0]
    got = np.array([t[1], t[2], t[3], t[4], t[5]]) / (t[0] + 1e-9)
    assert t[7] == 288 * 384 and np.allclose(got, G[f"{kind}_aee"], rtol=1e-6, atol=1e-9), (got, G[f"{kind}_aee"])
