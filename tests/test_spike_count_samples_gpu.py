"""The per-sample spike-count kernel (csrc/spike_count.hip: sdf_spike_count_seg_fwd, hip.spike_count_samples) against
`view.sum(dtype=int64)` per sample and step, exact.  Every view is carved out of a larger buffer whose other bytes are all 255 - in
front of an unaligned base, between the rows of a strided view, behind the end - and the samples themselves are random 0 / 1 bytes
lying side by side: a read across a piece boundary moves a count to a neighbouring sample, a read outside the view adds 255s."""
import pytest
import torch

from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 256 * 8 * 16          # bytes of a run one workgroup of the dense kernel reads (csrc/spike_count.hip: kScTileVecs vectors)
CALLS, TMAX = 3, 64          # the count block of the tests: (samples, CALLS, TMAX), the call under test is CALL
CALL = 1


def carve(s_out, T, s_in, rows, C, row_stride=None, base=0, seed=0, high=2):
    """-> (view (s_out, T, s_in, rows, C) u8 of random bytes below `high` inside a buffer of 255s, starting `base` bytes behind a
    256-byte boundary, reference sums (s_out * s_in, T) int64)."""
    rs = C if row_stride is None else row_stride
    span = s_out * T * s_in * rows * rs
    buf = torch.full((256 + base + span + 256,), 255, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    view = buf.as_strided((s_out, T, s_in, rows, C), (T * s_in * rows * rs, s_in * rows * rs, rows * rs, rs, 1), 256 + base)
    g = torch.Generator(device="cpu").manual_seed(seed)
    view.copy_(torch.randint(0, high, (s_out, T, s_in, rows, C), generator=g, dtype=torch.uint8))
    want = view.sum(dim=(3, 4), dtype=torch.int64).permute(0, 2, 1).reshape(s_out * s_in, T)
    return view, want


def handed_over(view):
    """The view as the engine hands it over: (spikes, t_dim, samples) - samples on dim 0 with the steps on dim 1 (s_in = 1), or the
    steps on dim 0 and the samples as consecutive pieces of every step's rows (s_out = 1)."""
    s_out, T, s_in, rows, C = view.shape
    if s_in == 1:
        return view[:, :, 0], 1, s_out
    assert s_out == 1
    return view[0].reshape(T, s_in * rows, C) if view.stride(3) == C else \
        view[0].as_strided((T, s_in * rows, C), (view.stride(1), view.stride(3), 1)), 0, s_in


def block(samples, fill=3):
    """A (samples, CALLS, TMAX) count block holding `fill`, inside a buffer of guard words."""
    buf = torch.full((5 + samples * CALLS * TMAX + 5,), -7, dtype=torch.int64, device=DEV)
    blk = buf[5:5 + samples * CALLS * TMAX].view(samples, CALLS, TMAX)
    blk.fill_(fill)
    return buf, blk


def count_into_block(view):
    """One call into [:, CALL, :T] of a fresh block: through the binding, or - samples on BOTH sides of the time axis, which no record
    of the engine has - through the C ABI with the descriptor written out."""
    s_out, T, s_in, rows, C = view.shape
    buf, blk = block(s_out * s_in)
    dst = blk[:, CALL, :T]
    with hip.launch_log() as log:
        if s_out > 1 and s_in > 1:
            d = hip.SpikeCountSegDesc()
            d.spikes, d.counts = view.data_ptr(), dst.data_ptr()
            d.s_out, d.T, d.s_in, d.rows, d.C, d.row_stride, d.sample_pitch = s_out, T, s_in, rows, C, view.stride(3), CALLS * TMAX
            assert hip.lib().sdf_spike_count_seg_fwd(d, hip._stream()) == 0
        else:
            spikes, t_dim, samples = handed_over(view)
            assert spikes.data_ptr() == view.data_ptr()                        # a view, not a copy
            out = hip.spike_count_samples(spikes, t_dim, samples, dst)
            assert out.data_ptr() == dst.data_ptr()
    return buf, blk, log


def check_block(buf, blk, want, fill=3):
    """Only [sample, CALL, :T] changed, by the reference sums (the call ADDS); the rest of the block and the guard words are whole."""
    T = want.shape[1]
    assert torch.equal(blk[:, CALL, :T], want + fill), (blk[:, CALL, :T].tolist(), (want + fill).tolist())
    rest = blk.clone()
    rest[:, CALL, :T] = fill
    assert bool((rest == fill).all())
    assert buf[:5].tolist() == [-7] * 5 and buf[-5:].tolist() == [-7] * 5


SHAPES = [(1, 2, 3, 7, 5),                     # pieces of 35 bytes: shorter than the head / tail logic's vectors, every boundary unaligned
          (3, 10, 1, 33, 96),                  # samples outside time
          (1, 2, 10, 324, 96),                 # a stage-0 window record of 10 replicas
          (2, 1, 2, 1, 1),                     # one byte per piece, samples on both sides
          (1, 64, 2, 3, 17),                   # T = 64
          (1, 1, 2, 1, TILE + 17)]             # 32 KiB + 17 bytes per piece: a second workgroup for its last vector and tail


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("base", [0, 1, 15])
def test_dense_pieces_at_every_base_offset(shape, base):
    view, want = carve(*shape, base=base, seed=sum(shape) + base)
    if shape[3] * shape[4] >= 16:
        assert not torch.equal(want[0], want[-1])                            # the samples differ: a wrong split would show
    buf, blk, log = count_into_block(view)
    check_block(buf, blk, want)
    assert len(log.rows) == 1 and "spike_count_seg_run_kernel" in log.rows[0][0], log.rows
    run = shape[3] * shape[4]
    assert log.rows[0][1] == shape[0] * shape[1] * shape[2] * max(1, -(-(run // 16) // (256 * 8)))
    buf2, blk2, _ = count_into_block(view)                                   # the same bits on a second run
    assert torch.equal(buf, buf2)


@pytest.mark.parametrize("base", [0, 1, 15])
def test_the_value_255_is_a_byte_like_any_other(base):
    """The sums are of bytes, not of bits: a piece of all 255 beside a piece of zeros."""
    view, want = carve(1, 2, 3, 7, 5, base=base, seed=base, high=256)
    view[0, :, 1] = 255
    view[0, :, 2] = 0
    want = view.sum(dim=(3, 4), dtype=torch.int64).permute(0, 2, 1).reshape(3, 2)
    assert want[1].tolist() == [255 * 35] * 2 and want[2].tolist() == [0, 0]
    buf, blk, _ = count_into_block(view)
    check_block(buf, blk, want)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("base", [0, 1, 15])
def test_strided_rows_on_both_halves_of_a_stacked_buffer(half, base):
    """(1, 2, 3, 50, 96) with row_stride 192: the q half and the k half (96 bytes in) of a q | k buffer holding 3 samples."""
    view, want = carve(1, 2, 3, 50, 96, row_stride=192, base=base + 96 * half, seed=20 + half)
    buf, blk, log = count_into_block(view)
    check_block(buf, blk, want)
    assert len(log.rows) == 1 and "spike_count_seg_rows_kernel" in log.rows[0][0], log.rows
    buf2, _, _ = count_into_block(view)
    assert torch.equal(buf, buf2)


def test_strided_samples_outside_time_and_the_padded_gate_record():
    view, want = carve(3, 10, 1, 30, 2, row_stride=208, base=13, seed=31)            # a channel slice of (B, D, h, w, 208)
    buf, blk, _ = count_into_block(view)
    check_block(buf, blk, want)
    n = 4 * 81 * 3 + 1                                                               # the token gate's (T', R, n) of a (T', R, n4) buffer
    view, want = carve(1, 2, 3, 1, n, row_stride=n + 3, seed=32)
    spikes = view[0, :, :, 0]
    assert hip.spike_count_samples_form(spikes, 0, 3) == (1, 2, 3, 1, n, n + 3)
    buf, blk = block(3)
    hip.spike_count_samples(spikes, 0, 3, blk[:, CALL, :2])
    check_block(buf, blk, want)


def test_one_sample_equals_the_single_sample_kernel():
    for shape, rs in (((1, 10, 1, 7, 17), None), ((1, 10, 1, 7, 17), 34), ((1, 2, 1, 324, 96), 192)):
        view, want = carve(*shape, row_stride=rs, base=5, seed=41)
        spikes = view[0, :, 0]
        one = hip.spike_count(spikes, 0)
        got = hip.spike_count_samples(spikes, 0, 1, torch.zeros((1, shape[1]), dtype=torch.int64, device=DEV))
        assert torch.equal(got[0], one) and torch.equal(one, want[0])


def test_binding_refusals_on_the_device():
    u8 = torch.zeros((3, 10, 7, 17), dtype=torch.uint8, device=DEV)
    ok = torch.zeros((3, 10), dtype=torch.int64, device=DEV)
    hip.spike_count_samples(u8, 1, 3, ok)
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(u8.float(), 1, 3, ok)                                     # not u8
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(u8, 1, 3, torch.zeros((3, 9), dtype=torch.int64, device=DEV))
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(u8, 1, 3, torch.zeros((3, 10), dtype=torch.int32, device=DEV))
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(u8, 1, 3, torch.zeros((10, 3), dtype=torch.int64, device=DEV).t())     # steps not dense
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(u8, 1, 3, torch.zeros((3, 20), dtype=torch.int64, device=DEV)[:, ::2])
    with pytest.raises(hip.SdfError):
        hip.spike_count_samples(torch.zeros((3, 65, 4, 4), dtype=torch.uint8, device=DEV), 1, 3,
                                torch.zeros((3, 65), dtype=torch.int64, device=DEV))      # T > 64: refused by the library
