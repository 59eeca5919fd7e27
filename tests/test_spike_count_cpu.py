"""CPU-side checks of the spike-count entry point (sdf_spike_count_fwd, the firing-rate monitor's kernel): the header, the signature
table and the Structure mirror agree on the new names, every argument error is refused before any launch (dummy pointers: no GPU is
touched), the binding refuses what it cannot count in place, and the ABI version did not move."""
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
    assert re.search(r"^int sdf_spike_count_fwd\(const SdfSpikeCountDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert list(hip.SIGNATURES)[-1] == "sdf_spike_count_fwd"                 # the header's position: its last prototype
    assert re.findall(r"^(?:int|int64_t|void) (sdf_\w+)\(", hdr, flags=re.M)[-1] == "sdf_spike_count_fwd"
    assert hip.SIGNATURES["sdf_spike_count_fwd"] == (C.c_int, (C.POINTER(hip.SpikeCountDesc), C.c_void_p))
    body = re.search(r"typedef struct SdfSpikeCountDesc \{(.*?)\} SdfSpikeCountDesc;", hdr, flags=re.S).group(1)
    members = [re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", d).groups() for d in body.split(";")[:-1]]
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    want = [(name, C.c_void_p if ptr else ctype[base]) for base, ptr, name in members]
    assert [n for n, _ in want] == ["spikes", "outer", "T", "rows", "C", "row_stride", "counts"]
    assert hip.SpikeCountDesc._fields_ == want


def test_version_is_still_107():
    assert loaded_lib().sdf_version() == 107
    assert re.search(r"#define SDF_VERSION 107\b", open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read())


def _desc(**kw):
    d = hip.SpikeCountDesc()
    d.spikes, d.counts = 0x10000, 0x20000
    d.outer, d.T, d.rows, d.C, d.row_stride = 1, 10, 7, 17, 17
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_are_refused_before_any_launch():
    lib = loaded_lib()
    call = lambda **kw: lib.sdf_spike_count_fwd(C.byref(_desc(**kw)), None)
    assert lib.sdf_spike_count_fwd(None, None) == E_NULL
    assert call(spikes=None) == E_NULL
    assert call(counts=None) == E_NULL
    for field in ("outer", "rows", "C"):
        assert call(**{field: 0}) == E_SHAPE, field
        assert call(**{field: -3}) == E_SHAPE, field
    assert call(T=0) == E_SHAPE
    assert call(T=65) == E_SHAPE
    assert call(row_stride=16) == E_SHAPE                        # row_stride < C
    assert call(counts=0x20004) == E_ALIGN                       # counts not 8-byte aligned
    # NULL comes before shape, shape before alignment (the header's order of the checks)
    assert call(spikes=None, T=0) == E_NULL
    assert call(T=0, counts=0x20004) == E_SHAPE


def test_binding_refuses_cpu_tensors_and_what_it_cannot_count_in_place():
    with pytest.raises(hip.SdfError, match="device tensor"):
        hip.spike_count(torch.zeros((10, 4, 8), dtype=torch.uint8), 0)
    with pytest.raises(hip.SdfError):
        hip.spike_count([[0, 1]], 0)


def test_addressing_form_of_views():
    """spike_count_form is host arithmetic on shapes and strides: the forms the engine hands to the monitor, and the refusals."""
    form = hip.spike_count_form
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    assert form(u8(10, 7, 17), 0) == (1, 10, 7, 17, 17)                               # contiguous (T, rows, C)
    assert form(u8(2, 10, 5, 6, 96), 1) == (2, 10, 30, 96, 96)                        # channel-last (B, D, h, w, C)
    assert form(u8(2, 10, 5, 6, 208)[..., 13:15], 1) == (2, 10, 30, 2, 208)           # channel slice, odd c0
    qk = u8(2 * 81 * 4, 192)
    assert form(qk[:, :96].reshape(2, 81 * 4, 96), 0) == (1, 2, 324, 96, 192)         # the q half of a stacked q | k buffer
    assert form(qk[:, 96:].reshape(2, 81 * 4, 96), 0) == (1, 2, 324, 96, 192)
    assert form(u8(2, 972)[:, :970], 0) == (1, 2, 1, 970, 972)                        # one row per step, padded pitch
    assert form(u8(1, 1, 1, 1), 1) == (1, 1, 1, 1, 1)
    with pytest.raises(hip.SdfError):
        form(u8(10, 7, 17), 2)                                                        # step axis is dim 0 or 1
    with pytest.raises(hip.SdfError):
        form(u8(10, 7, 17).permute(1, 0, 2), 1)                                       # steps not rows x stride apart
    with pytest.raises(hip.SdfError):
        form(u8(10, 4, 6, 8)[:, :, :5], 0)                                            # two row strides
    with pytest.raises(hip.SdfError):
        form(u8(1, 7, 17).expand(10, 7, 17), 0)                                       # stride 0
    with pytest.raises(hip.SdfError):
        form(u8(0, 7, 17), 0)
