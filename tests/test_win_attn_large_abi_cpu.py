"""CPU-side checks of sdf_win_attn_large_fwd (csrc/win_attn_large.hip), the window-attention forward for 192 < N <= 1024 tokens per
window: the symbol is exported and bound, its range is refused on both sides, and every argument error of sdf_win_attn_fwd's
dispatcher returns the same code from it - with dummy pointers, so everything is refused before any launch and no GPU is needed.
sdf_win_attn_fwd itself keeps refusing more than 192 tokens."""
import ctypes as C
import os

from sdformerflow_amd import hip

E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
P = 0x10000


def loaded_lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def desc(mode=0, **kw):
    d = hip.WinAttnDesc()
    d.mode, d.q, d.k, d.v, d.out, d.scale, d.bias = mode, P, P, P, P, P, P
    d.B_, d.nW, d.nH, d.N, d.hd, d.Tq, d.N1 = 4, 1, 3, 450, 32, 2, 225            # (valid in both modes but for **kw)
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def test_symbol_is_exported_and_bound():
    lib = loaded_lib()
    assert "sdf_win_attn_large_fwd" in hip.SIGNATURES
    assert hip.SIGNATURES["sdf_win_attn_large_fwd"] == hip.SIGNATURES["sdf_win_attn_fwd"]
    f = lib.sdf_win_attn_large_fwd
    assert f.restype is C.c_int and tuple(f.argtypes) == (C.POINTER(hip.WinAttnDesc), C.c_void_p)
    assert lib.sdf_win_attn_large_fwd(None, None) == E_NULL


def test_range_is_192_exclusive_to_1024_inclusive():
    lib = loaded_lib()
    large = lambda **kw: lib.sdf_win_attn_large_fwd(C.byref(desc(**kw)), None)
    assert large(N=192, N1=96) == E_SHAPE                       # sdf_win_attn_fwd's sizes
    assert large(N=162, N1=81) == E_SHAPE
    assert large(N=1025, Tq=1, N1=1025) == E_SHAPE
    assert large(mode=1, N=192, N1=96) == E_SHAPE and large(mode=1, N=1025, Tq=1, N1=1025) == E_SHAPE
    assert large(N=0) == E_SHAPE and large(N=-5) == E_SHAPE
    # the first entry point is unchanged: 193 tokens and beyond are refused there
    assert lib.sdf_win_attn_fwd(C.byref(desc(N=193, Tq=1, N1=193)), None) == E_SHAPE
    assert lib.sdf_win_attn_fwd(C.byref(desc(N=450)), None) == E_SHAPE
    assert lib.sdf_win_attn_fwd(C.byref(desc(mode=1, N=450)), None) == E_SHAPE


def test_argument_errors_equal_those_of_the_first_entry_point():
    """The cases of tests/test_abi_cpu.py::test_win_attn_fwd_refuses_what_its_kernels_cannot_serve and the NULL / selector / head-dim
    cases of test_argument_errors_are_reported_before_any_launch, at N = 450 (Tq = 2, N1 = 225)."""
    lib = loaded_lib()
    refused = lambda mode=0, **kw: lib.sdf_win_attn_large_fwd(C.byref(desc(mode, **kw)), None)
    assert refused(mask=P, nW=3) == E_SHAPE                     # B_ % nW != 0
    assert refused(mask=P, nW=0) == E_SHAPE                     # nW < 1
    assert refused(mode=1, mask=P, nW=3) == E_SHAPE
    assert refused(mode=1, N1=224) == E_SHAPE                   # Tq * N1 != N
    assert refused(mode=1, Tq=0, N1=450) == E_SHAPE             # Tq < 1
    assert refused(mode=1, row_map=P, pad_qkv=P) == E_NULL      # the row map is the windowed ANN form
    assert refused(row_map=P) == E_NULL                         # ... and needs the pad row
    assert refused(q=P + 8) == E_ALIGN                          # ANN q: float4 loads
    assert refused(mode=1, q=P + 2) == E_ALIGN                  # SEW q: 4 spikes per load
    assert refused(out=P + 2) == E_ALIGN
    assert refused(hd=16) == E_SHAPE                            # head dim must be 32
    assert refused(mode=5) == E_DTYPE
    assert refused(bias=None) == E_NULL
    assert refused(B_=0) == E_SHAPE and refused(nH=0) == E_SHAPE
    # the order of the checks: NULL before the selector before the shape before the alignment
    assert refused(mode=5, bias=None, N=100, q=P + 2) == E_NULL
    assert refused(mode=5, N=100, q=P + 2) == E_DTYPE
    assert refused(N=100, q=P + 2) == E_SHAPE
    # the same descriptors, at a size the first entry point serves, get the same codes there
    first = lambda mode=0, **kw: lib.sdf_win_attn_fwd(C.byref(desc(mode, **dict({"N": 162, "N1": 81}, **kw))), None)
    for kw, code in (({"mask": P, "nW": 3}, E_SHAPE), ({"mode": 1, "Tq": 0, "N1": 162}, E_SHAPE), ({"row_map": P}, E_NULL),
                     ({"q": P + 8}, E_ALIGN), ({"hd": 16}, E_SHAPE), ({"mode": 5}, E_DTYPE), ({"bias": None}, E_NULL)):
        big = dict(kw)
        if big.get("N1") == 162:
            big["N1"] = 450
        assert first(**kw) == refused(**big) == code, kw


def test_wrappers_pick_the_entry_point_by_window_size(monkeypatch):
    """hip.win_attn_ann / _windowed / _sew go through one helper: up to 192 tokens the first entry point, beyond it the new one."""
    loaded_lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            return lambda *a: (calls.append(name), 0)[1]
    monkeypatch.setattr(hip, "lib", lambda: Spy())
    monkeypatch.setattr(hip, "_stream", lambda: None)
    for N, want in ((162, "sdf_win_attn_fwd"), (192, "sdf_win_attn_fwd"), (193, "sdf_win_attn_large_fwd"), (450, "sdf_win_attn_large_fwd"),
                    (1024, "sdf_win_attn_large_fwd"), (1025, "sdf_win_attn_large_fwd")):
        hip._win_attn_fwd(desc(N=N))
    assert calls == ["sdf_win_attn_fwd"] * 2 + ["sdf_win_attn_large_fwd"] * 4
