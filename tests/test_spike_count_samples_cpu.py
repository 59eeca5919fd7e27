"""CPU-side checks of the per-sample spike-count entry point (sdf_spike_count_seg_fwd, the replica firing-rate monitor's kernel): the
header, the signature table and the Structure mirror agree field for field, the existing entry point kept its place and the ABI
version did not move, every argument error is refused before any launch (dummy pointers: no GPU is touched), and
hip.spike_count_samples_form - host arithmetic - gives the addressing form of the records the engine hands over and refuses the rest."""
import ctypes as C
import os
import re

import pytest
import torch

from sdformerflow_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


def loaded_lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def header():
    src = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_header_signature_table_and_structure_agree():
    hdr = header()
    assert re.search(r"^int sdf_spike_count_seg_fwd\(const SdfSpikeCountSegDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert hip.SIGNATURES["sdf_spike_count_seg_fwd"] == (C.c_int, (C.POINTER(hip.SpikeCountSegDesc), C.c_void_p))
    body = re.search(r"typedef struct SdfSpikeCountSegDesc \{(.*?)\} SdfSpikeCountSegDesc;", hdr, flags=re.S).group(1)
    members = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in body.split(";")[:-1]]
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    want = [(name, C.c_void_p if ptr else ctype[base]) for base, ptr, name in members]
    assert [n for n, _ in want] == ["spikes", "s_out", "T", "s_in", "rows", "C", "row_stride", "counts", "sample_pitch"]
    assert hip.SpikeCountSegDesc._fields_ == want


def test_the_existing_entry_point_is_still_last_and_the_version_still_107():
    protos = re.findall(r"^(?:int|int64_t|void) (sdf_\w+)\(", header(), flags=re.M)
    assert protos[-2:] == ["sdf_spike_count_seg_fwd", "sdf_spike_count_fwd"]            # the new entry in front of that section
    assert list(hip.SIGNATURES)[-2:] == ["sdf_spike_count_seg_fwd", "sdf_spike_count_fwd"]
    assert hip.SpikeCountDesc._fields_ == [("spikes", C.c_void_p), ("outer", C.c_int64), ("T", C.c_int), ("rows", C.c_int64),
                                           ("C", C.c_int), ("row_stride", C.c_int64), ("counts", C.c_void_p)]
    assert loaded_lib().sdf_version() == 107
    assert re.search(r"#define SDF_VERSION 107\b", open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read())


def _desc(**kw):
    d = hip.SpikeCountSegDesc()
    d.spikes, d.counts = 0x10000, 0x20000
    d.s_out, d.T, d.s_in, d.rows, d.C, d.row_stride, d.sample_pitch = 1, 10, 3, 7, 17, 17, 10
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_are_refused_before_any_launch():
    lib = loaded_lib()
    call = lambda **kw: lib.sdf_spike_count_seg_fwd(C.byref(_desc(**kw)), None)
    assert lib.sdf_spike_count_seg_fwd(None, None) == E_NULL
    assert call(spikes=None) == E_NULL
    assert call(counts=None) == E_NULL
    for field in ("s_out", "s_in", "rows", "C"):
        assert call(**{field: 0}) == E_SHAPE, field
        assert call(**{field: -3}) == E_SHAPE, field
    assert call(T=0) == E_SHAPE
    assert call(T=65, sample_pitch=65) == E_SHAPE
    assert call(row_stride=16) == E_SHAPE                        # row_stride < C
    assert call(sample_pitch=9) == E_SHAPE                       # sample_pitch < T
    assert call(counts=0x20004) == E_ALIGN                       # counts not 8-byte aligned
    # NULL comes before shape, shape before alignment (the header's order of the checks)
    assert call(spikes=None, T=0) == E_NULL
    assert call(s_in=0, counts=0x20004) == E_SHAPE
    # beyond 2^31 workgroups / 2^62 bytes
    assert call(s_out=1 << 30, s_in=1 << 30) == E_SHAPE
    assert call(rows=1 << 40, row_stride=1 << 30, C=1) == E_SHAPE
    assert call(sample_pitch=1 << 60) == E_SHAPE


def test_addressing_form_of_the_records_the_engine_hands_over():
    """(s_out, T, s_in, rows, C, row_stride): samples outside time for the channel-last records (step axis 1), inside it - R equal
    consecutive pieces of every time block - for the window records (step axis 0)."""
    form = hip.spike_count_samples_form
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    R, nW, N1 = 3, 4, 81
    assert form(u8(R, 10, 36, 48, 96), 1, R) == (R, 10, 1, 36 * 48, 96, 96)                       # a channel-last (B, D, h, w, C) record
    assert form(u8(R, 10, 5, 6, 208)[..., :100], 1, R) == (R, 10, 1, 30, 100, 208)                # the decoder's channel slice
    assert form(u8(2, R * nW * N1, 96), 0, R) == (1, 2, R, nW * N1, 96, 96)                       # proj_sn / attn_sn: (T', R nW N1, C)
    assert form(u8(2, R * nW, N1, 96), 0, R) == (1, 2, R, nW * N1, 96, 96)
    qk = u8(2 * R * nW * N1, 192)
    assert form(qk[:, :96].reshape(2, R * nW * N1, 96), 0, R) == (1, 2, R, nW * N1, 96, 192)      # the q half of a stacked q | k buffer
    assert form(qk[:, 96:].reshape(2, R * nW * N1, 96), 0, R) == (1, 2, R, nW * N1, 96, 192)
    n = nW * N1 * 3 + 1                                                                           # the token gate, padded per sample
    assert form(u8(2, R, n + 3)[:, :, :n], 0, R) == (1, 2, R, 1, n, n + 3)
    assert form(u8(10, R, 18, 24, 384), 0, R) == (1, 10, R, 18 * 24, 384, 384)                    # the patch merging's (D, B, H2, W2, 4C)
    assert form(u8(10, 7, 17), 0, 1) == (1, 10, 1, 7, 17, 17)                                     # one sample: spike_count's form
    assert form(u8(1, 10, 7, 17), 1, 1) == (1, 10, 1, 7, 17, 17)


def test_addressing_form_refusals():
    form = hip.spike_count_samples_form
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    with pytest.raises(hip.SdfError, match="equal consecutive pieces"):
        form(u8(2, 4 * 81, 96), 0, 5)                                                 # 324 rows of a step do not split into 5 samples
    with pytest.raises(hip.SdfError):
        form(u8(3, 10, 7, 17), 1, 2)                                                  # samples outside time are dim 0: 3, not 2
    with pytest.raises(hip.SdfError):
        form(u8(10, 7, 17).permute(1, 0, 2), 1, 7)                                    # a permuted view: steps not rows x stride apart
    with pytest.raises(hip.SdfError):
        form(u8(10, 4, 6, 8)[:, :, :5], 0, 2)                                         # two row strides
    with pytest.raises(hip.SdfError):
        form(torch.zeros((3, 10, 7, 17), dtype=torch.float32), 1, 3)                  # fp32: spikes are u8
    with pytest.raises(hip.SdfError):
        form(u8(3, 10, 7, 17), 1, 0)
    with pytest.raises(hip.SdfError):
        form(u8(3, 10, 7, 17), 2, 3)                                                  # step axis is dim 0 or 1


def test_binding_refuses_cpu_tensors():
    with pytest.raises(hip.SdfError, match="device tensor"):
        hip.spike_count_samples(torch.zeros((3, 10, 4, 8), dtype=torch.uint8), 1, 3, torch.zeros((3, 10), dtype=torch.int64))
