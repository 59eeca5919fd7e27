"""The membrane-statistics kernel (csrc/membrane_stats.hip, hip.membrane_stats) against its numpy restatement
(monitor.membrane_record), integer for integer.

Values: random membranes plus, planted at known places, +0, -0, a denormal, +-inf, NaN, a value exactly on `lo`, on `hi` and on an
inner edge, and values whose rintf(x * 65536) is a tie.  Every view is carved out of a larger buffer whose other floats are all NaN -
in front of an unaligned base, behind a ragged end, between the rows of a strided view - so a read outside the view shows up in
n_nan."""
import numpy as np
import pytest
import torch

from sdformerflow_amd import hip
from sdformerflow_amd.monitor import membrane_record, membrane_unkey

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO, HI = -0.2, 0.2
TILE = 256 * 8 * 4            # floats of a run one workgroup of the contiguous kernel reads (kMsTileVecs vectors)
SPECIAL = [0.0, -0.0, 1e-41, -1e-41, float("inf"), float("-inf"), float("nan"), LO, HI, 0.0 + (HI - LO) / 4 + LO,
           0.5 / 65536, 1.5 / 65536, -2.5 / 65536, 40000.0, -40000.0]


def carve(outer, T, rows, C, row_stride=None, base=0, seed=0):
    """-> view (outer, T, rows, C) fp32 inside a buffer of NaNs, starting `base` BYTES behind a 256-byte boundary; random membranes in
    (-0.35, 0.35) with the special values planted from element 0 on (as far as they fit) and at the end of the last step."""
    rs = C if row_stride is None else row_stride
    span = outer * T * rows * rs
    buf = torch.full((64 + base // 4 + span + 64,), float("nan"), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 256 == 0 and base % 4 == 0
    view = buf.as_strided((outer, T, rows, C), (T * rows * rs, rows * rs, rs, 1), 64 + base // 4)
    g = torch.Generator(device="cpu").manual_seed(seed)
    vals = torch.rand((outer, T, rows, C), generator=g) * 0.7 - 0.35
    flat = vals.view(-1)
    k = min(len(SPECIAL), flat.numel())
    flat[:k] = torch.tensor(SPECIAL[:k])
    if flat.numel() >= 3 * len(SPECIAL):
        flat[-len(SPECIAL):] = torch.tensor(SPECIAL)
    view.copy_(vals)
    return view, vals


def want_table(vals, bins):
    """numpy records of (outer, T, rows, C) values: the steps on axis 1."""
    a = vals.numpy()
    return membrane_record(np.moveaxis(a, 1, 0).reshape(a.shape[1], -1), LO, HI, bins)


def stats(view, bins, table=None):
    return hip.membrane_stats(view[0], 0, table, LO, HI, bins) if view.shape[0] == 1 else hip.membrane_stats(view, 1, table, LO, HI, bins)


def assert_equal(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), [(t, got[t, :4].tolist(), want[t, :4].tolist()) for t in range(len(want)) if not np.array_equal(got[t], want[t])][:3]


@pytest.mark.parametrize("run", [1, 3, 4, 5, 1028, TILE + 1028 + 3])
@pytest.mark.parametrize("base", [0, 4, 12])
def test_contiguous_runs_at_every_base_offset(run, base):
    """row_stride == C: one run per (o, t) at 0, 4 and 12 bytes from a 16-byte boundary; runs shorter than a vector, ragged, and larger
    than one workgroup's tile."""
    T = 2 if run > TILE else 10
    view, vals = carve(1, T, 1, run, base=base, seed=run + base)
    with hip.launch_log() as log:
        got = stats(view, 64)
    assert len(log.rows) == 1 and "membrane_stats_run_kernel" in log.rows[0][0], log.rows
    assert_equal(got, want_table(vals, 64))


@pytest.mark.parametrize("T", [1, 2, 10])
@pytest.mark.parametrize("bins", [1, 64, 256])
def test_steps_and_bins(T, bins):
    view, vals = carve(2, T, 7, 33, base=4, seed=T + bins)
    got = stats(view, bins)
    want = want_table(vals, bins)
    assert_equal(got, want)
    assert int(want[:, 0].sum()) >= 1 and int(want[:, 4].sum()) >= 1 and int(want[:, 4 + bins + 1].sum()) >= 1     # NaN, under- and overflow


@pytest.mark.parametrize("shape,row_stride,base", [((1, 10, 7, 32), 64, 0), ((2, 10, 5, 32), 64, 128), ((1, 2, 300, 32), 64, 4),
                                                   ((2, 10, 30, 2), 208, 52)])
def test_strided_rows(shape, row_stride, base):
    """row_stride = 2 C at C = 32 (both halves of a stacked buffer, one of them more than a workgroup tile per step) and a 2-channel
    slice of a 208-channel activation: the floats between the rows are NaN and stay out of the result."""
    view, vals = carve(*shape, row_stride=row_stride, base=base, seed=row_stride + base)
    with hip.launch_log() as log:
        got = stats(view, 64)
    assert len(log.rows) == 1 and "membrane_stats_rows_kernel" in log.rows[0][0], log.rows
    assert_equal(got, want_table(vals, 64))


def test_a_second_call_doubles_the_counts_and_keeps_the_extremes():
    view, vals = carve(2, 10, 5, 96, seed=3)
    table = stats(view, 64)
    first = table.clone()
    assert stats(view, 64, table) is table
    want = want_table(vals, 64)
    assert_equal(first, want)
    twice = want.copy()
    twice[:, :2] *= 2
    twice[:, 4:] *= 2
    assert_equal(table, twice)


def test_special_values_land_where_the_restatement_says():
    """The planted values in one step, read back through the monitor's decoding: extremes are the exact floats, -0 sorts below +0."""
    vals = torch.tensor(SPECIAL).view(1, 1, 1, -1)
    view = torch.full((64 + vals.numel() + 64,), float("nan"), device=DEV)[64:64 + vals.numel()].view(1, 1, 1, -1)
    view.copy_(vals)
    rec = stats(view, 4).cpu().numpy()[0]
    assert rec[0] == 1                                                                  # the NaN, and none of the NaNs around the run
    assert membrane_unkey(rec[2])[()] == -np.inf and membrane_unkey(rec[3])[()] == np.inf
    q = lambda x: int(np.rint(np.clip(np.float32(x), -32768, 32768) * np.float32(65536)))
    assert rec[1] == sum(q(x) for x in SPECIAL if x == x) and q(0.5 / 65536) == 0 and q(1.5 / 65536) == 2 and q(-2.5 / 65536) == -2
    assert_equal(torch.from_numpy(rec[None]), membrane_record(vals.numpy().reshape(1, -1), LO, HI, 4))
    assert rec[4] == 2 and rec[4 + 5] == 3                                              # underflow; overflow = {hi, +inf, 40000}
    pair = torch.tensor([-0.0, 0.0], device=DEV).view(1, 1, 1, 2)
    r2 = stats(pair, 4).cpu().numpy()[0]
    assert membrane_unkey(r2[2]).view(np.uint32)[()] == 0x80000000 and membrane_unkey(r2[3]).view(np.uint32)[()] == 0


def test_refusals_before_any_launch():
    v = torch.zeros((10, 7, 17), device=DEV)
    with hip.launch_log() as log:
        for bad in (0, 257):
            with pytest.raises(hip.SdfError):
                hip.membrane_stats(v, 0, None, LO, HI, bad)
        with pytest.raises(hip.SdfError) as e:
            hip.membrane_stats(v, 0, None, 0.2, 0.2, 64)
        assert e.value.rc == hip.E_SHAPE
        with pytest.raises(hip.SdfError):
            hip.membrane_stats(v.to(torch.uint8), 0)
        with pytest.raises(hip.SdfError):
            hip.membrane_stats(v, 0, torch.zeros((10, 69), dtype=torch.int64, device=DEV))      # bins = 64 needs 70 columns
    assert log.rows == []
