"""The spike-count kernel (csrc/spike_count.hip, hip.spike_count) against `view.sum(dtype=int64)` per step, exact, on random 0 / 1
bytes.  Every view is carved out of a larger buffer whose other bytes are all 1 - the bytes beside a row, between the rows of a
strided view, in front of an unaligned base and behind a ragged end - so a read outside the view shows up as a wrong count."""
import pytest
import torch

from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256 * 8 * 16          # bytes of a run one workgroup of the contiguous kernel reads (csrc/spike_count.hip: kScTileVecs vectors)


def carve(outer, T, rows, C, row_stride=None, base=0, seed=0):
    """-> (view (outer, T, rows, C) u8 of random 0 / 1 inside a buffer of ones, starting `base` bytes behind a 256-byte boundary,
    per-step reference sums (T,) int64)."""
    rs = C if row_stride is None else row_stride
    span = outer * T * rows * rs
    buf = torch.ones(256 + base + span + 256, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf.as_strided((outer, T, rows, C), (T * rows * rs, rows * rs, rs, 1), 256 + base)
    g = torch.Generator(device="cpu").manual_seed(seed)
    view.copy_(torch.randint(0, 2, (outer, T, rows, C), generator=g, dtype=torch.uint8))
    return view, view.sum(dim=(0, 2, 3), dtype=torch.int64)


def count(view, counts=None):
    """The view as the engine would hand it over: (T, rows, C) with the steps on dim 0 when there is no batch, else steps on dim 1."""
    return hip.spike_count(view[0], 0, counts) if view.shape[0] == 1 else hip.spike_count(view, 1, counts)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 1, 15), (1, 10, 7, 17), (2, 10, 5, 96), (1, 20, 257, 33),
                                   (1, 2, 3, (3 * TILE + 5003) // 3), (2, 64, 1, TILE + 16)])
@pytest.mark.parametrize("base", [0, 1, 2, 3, 5])
def test_contiguous_runs_at_every_base_offset(shape, base):
    """row_stride == C: one run per (o, t); a run that is no multiple of 16 bytes, starts off a 16-byte boundary (every base, and every
    step's own offset when the run is odd) and spans several workgroup tiles plus a ragged tail."""
    view, want = carve(*shape, base=base, seed=sum(shape) + base)
    with hip.launch_log() as log:
        got = count(view)
    assert got.dtype == torch.int64 and got.shape == (shape[1],)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert len(log.rows) == 1 and "spike_count_run_kernel" in log.rows[0][0], log.rows
    run = shape[2] * shape[3]
    assert log.rows[0][1] == shape[0] * shape[1] * max(1, -(-(run // 16) // (256 * 8)))


def test_three_tiles_and_a_ragged_tail_is_what_the_large_case_spans():
    run = 3 * ((3 * TILE + 5003) // 3)
    assert run > 3 * TILE and run % 16 != 0 and (run // 16) % (256 * 8) != 0


@pytest.mark.parametrize("shape,row_stride,base", [((1, 10, 7, 17), 18, 0), ((1, 10, 7, 17), 34, 3), ((2, 10, 5, 96), 97, 1),
                                                   ((2, 10, 5, 96), 192, 96), ((2, 10, 30, 2), 208, 13), ((1, 2, 1, 970), 972, 0),
                                                   ((1, 2, 700, 96), 192, 96)])
def test_strided_rows(shape, row_stride, base):
    """row_stride = C + 1 and 2 C (the k half of a stacked q | k buffer starts C bytes in), a 2-channel slice at an odd channel of a
    208-channel activation, a padded pitch with one row per step, and a view of more than one workgroup tile per step."""
    view, want = carve(*shape, row_stride=row_stride, base=base, seed=row_stride)
    with hip.launch_log() as log:
        got = count(view)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert len(log.rows) == 1 and "spike_count_rows_kernel" in log.rows[0][0], log.rows


def test_engine_style_views_are_counted_in_place():
    """The views the engine hands over, made the way it makes them: a channel slice of a channel-last activation and both halves of a
    stacked (M, 2C) buffer at a 256-byte-rounded offset of a workspace."""
    g = torch.Generator(device="cpu").manual_seed(5)
    act = torch.randint(0, 2, (2, 10, 5, 6, 208), generator=g, dtype=torch.uint8).to(DEV)
    for sl in (slice(0, 100), slice(13, 15), slice(101, 208)):
        v = act[..., sl]
        assert torch.equal(hip.spike_count(v, 1), v.sum(dim=(0, 2, 3, 4), dtype=torch.int64))
    Tq, rows, Cc = 2, 4 * 81, 96
    M = Tq * rows
    ws = torch.ones(1 << 20, dtype=torch.uint8, device=DEV)
    off = (M * Cc + 255) // 256 * 256
    ws[off:off + M * 2 * Cc] = torch.randint(0, 2, (M * 2 * Cc,), generator=g, dtype=torch.uint8).to(DEV)
    qk = ws[off:][:M * 2 * Cc].view(M, 2 * Cc)
    for half in (qk[:, :Cc], qk[:, Cc:]):
        v = half.reshape(Tq, rows, Cc)
        assert v.data_ptr() in (qk.data_ptr(), qk.data_ptr() + Cc)                       # a view, not a copy
        assert torch.equal(hip.spike_count(v, 0), v.sum(dim=(1, 2), dtype=torch.int64))
    e = ws[:M * Cc - 7].view(1, -1)                                                        # the head of the workspace, ragged end
    assert int(hip.spike_count(e, 0)) == M * Cc - 7


def test_counts_accumulate_carry_into_the_high_word_and_leave_their_neighbours():
    view, want = carve(2, 10, 5, 96, base=3, seed=11)
    table = torch.full((14,), -7, dtype=torch.int64, device=DEV)
    table[2:12] = 0
    out = count(view, table[2:12])
    assert out.data_ptr() == table[2:12].data_ptr()
    assert torch.equal(table[2:12], want)
    count(view, table[2:12])                                     # a second call adds to the first
    assert torch.equal(table[2:12], 2 * want)
    assert table[:2].tolist() == [-7, -7] and table[12:].tolist() == [-7, -7]
    big = torch.full((10,), 1 << 40, dtype=torch.int64, device=DEV)
    count(view, big)
    assert torch.equal(big, want + (1 << 40))
    near = torch.full((10,), (1 << 32) - 1, dtype=torch.int64, device=DEV)      # the add carries out of the low word
    count(view, near)
    assert torch.equal(near, want + ((1 << 32) - 1))
    # a call with fewer steps than the table touches its own entries only
    v3, w3 = carve(1, 3, 1, 15, seed=12)
    t = torch.full((6,), 5, dtype=torch.int64, device=DEV)
    count(v3, t[1:4])
    assert t.tolist() == [5] + (w3 + 5).tolist() + [5, 5]


def test_binding_refusals_on_the_device():
    u8 = torch.zeros((10, 7, 17), dtype=torch.uint8, device=DEV)
    with pytest.raises(hip.SdfError):
        hip.spike_count(u8.float(), 0)                                        # not u8
    with pytest.raises(hip.SdfError):
        hip.spike_count(u8.permute(1, 0, 2), 1)                               # not in the addressing form: no .contiguous() behind it
    with pytest.raises(hip.SdfError):
        hip.spike_count(u8, 0, torch.zeros(9, dtype=torch.int64, device=DEV))    # counts of the wrong length
    with pytest.raises(hip.SdfError):
        hip.spike_count(u8, 0, torch.zeros(10, dtype=torch.int32, device=DEV))
    with pytest.raises(hip.SdfError):
        hip.spike_count(torch.zeros((65, 4, 4), dtype=torch.uint8, device=DEV), 0)   # T > 64: refused by the library
