"""CPU-side checks of sdf_win_attn_scores_fwd (csrc/win_attn_scores.hip), the attention map (B_, nH, N, N) of the window attention for
1 <= N <= 1024 tokens per window: the symbol is exported and bound, the hip.py table row equals the header's prototype, and every
argument error returns its code - with dummy pointers, so everything is refused before any launch and no GPU is needed.  The manner
of tests/test_win_attn_large_abi_cpu.py."""
import ctypes as C
import os
import re

from sdformerflow_amd import hip

E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
P = 0x10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def loaded_lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def desc(mode=0, **kw):
    d = hip.WinAttnDesc()
    d.mode, d.q, d.k, d.scale, d.bias = mode, P, P, P, P                          # (v and out stay NULL: the entry point ignores them)
    d.B_, d.nW, d.nH, d.N, d.hd, d.Tq, d.N1 = 4, 1, 3, 450, 32, 2, 225            # (valid in both modes but for **kw)
    for f, v in kw.items():
        setattr(d, f, v)
    return d


def refused(mode=0, scores=P, **kw):
    return loaded_lib().sdf_win_attn_scores_fwd(C.byref(desc(mode, **kw)), scores, None)


def test_symbol_is_exported_and_bound():
    lib = loaded_lib()
    assert "sdf_win_attn_scores_fwd" in hip.SIGNATURES
    f = lib.sdf_win_attn_scores_fwd
    assert f.restype is C.c_int and tuple(f.argtypes) == (C.POINTER(hip.WinAttnDesc), C.c_void_p, C.c_void_p)
    assert f(None, None, None) == E_NULL and f(None, P, None) == E_NULL


def test_table_row_equals_the_header_prototype():
    """`int sdf_win_attn_scores_fwd(const SdfWinAttnDesc* d, float* scores, void* stream);` read from the header, type by type."""
    txt = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    m = re.search(r"^(\w+)\s+sdf_win_attn_scores_fwd\(([^)]*)\);", txt, re.M)
    assert m, "no prototype in the header"
    ctype = {"int": C.c_int, "const SdfWinAttnDesc*": C.POINTER(hip.WinAttnDesc), "float*": C.c_void_p, "void*": C.c_void_p}
    args = tuple(ctype[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(2).split(","))
    assert [a.strip().rsplit(" ", 1)[1] for a in m.group(2).split(",")] == ["d", "scores", "stream"]
    assert hip.SIGNATURES["sdf_win_attn_scores_fwd"] == (ctype[m.group(1)], args)


def test_null_pointers():
    assert refused(q=None) == E_NULL
    assert refused(scale=None) == E_NULL
    assert refused(bias=None) == E_NULL
    assert refused(mode=1, k=None) == E_NULL                    # SEW reads k ...
    assert refused(k=None, scores=None) == E_NULL               # (ANN does not: what is left is the NULL scores)
    assert refused(row_map=P) == E_NULL                         # the row map needs the pad row
    assert refused(scores=None) == E_NULL
    assert refused(mode=1, scores=None) == E_NULL


def test_ignored_fields_may_be_null_and_valid_descriptors_reach_the_alignment_check():
    """v and out are NULL in every descriptor of this file; with everything else valid the last check is the alignment of `scores`
    (an odd address: refused there, still before any launch)."""
    assert refused(scores=P + 2) == E_ALIGN
    assert refused(mode=1, scores=P + 1) == E_ALIGN
    assert refused(k=None, scores=P + 2) == E_ALIGN             # ANN without k
    assert refused(row_map=P, pad_qkv=P, scores=P + 2) == E_ALIGN
    assert refused(mask=P, nW=2, scores=P + 2) == E_ALIGN
    for N, Tq, N1 in ((1, 1, 1), (18, 2, 9), (162, 2, 81), (192, 2, 96), (193, 1, 193), (1024, 2, 512)):   # one design for the whole range
        assert refused(N=N, Tq=Tq, N1=N1, scores=P + 2) == E_ALIGN
        assert refused(mode=1, N=N, Tq=Tq, N1=N1, scores=P + 2) == E_ALIGN
    assert refused(q=P + 8) == E_ALIGN                          # ANN q: float4 loads, as sdf_win_attn_fwd
    assert refused(mode=1, q=P + 2) == E_ALIGN                  # SEW q: 4 spikes per load


def test_selector_and_shapes():
    assert refused(mode=5) == E_DTYPE and refused(mode=-1) == E_DTYPE
    assert refused(hd=16) == E_SHAPE                            # head dim must be 32
    assert refused(B_=0) == E_SHAPE and refused(nH=0) == E_SHAPE
    assert refused(N=0) == E_SHAPE and refused(N=-5) == E_SHAPE
    assert refused(N=1025) == E_SHAPE and refused(mode=1, N=1025, Tq=1, N1=1025) == E_SHAPE
    assert refused(mode=1, N1=224) == E_SHAPE                   # Tq * N1 != N
    assert refused(mode=1, Tq=0, N1=450) == E_SHAPE             # Tq < 1
    assert refused(mask=P, nW=3) == E_SHAPE                     # B_ % nW != 0
    assert refused(mask=P, nW=0) == E_SHAPE                     # nW < 1
    assert refused(mode=1, mask=P, nW=3) == E_SHAPE
    assert refused(mode=1, row_map=P, pad_qkv=P) == E_SHAPE     # the row map is the windowed ANN form


def test_order_of_the_checks():
    """NULL before the selector before the shape before `scores` (NULL, then alignment)."""
    assert refused(mode=5, bias=None, N=2000, scores=None) == E_NULL
    assert refused(mode=5, N=2000, scores=None) == E_DTYPE
    assert refused(N=2000, scores=None) == E_SHAPE
    assert refused(N=2000, scores=P + 2) == E_SHAPE
    assert refused(scores=None, q=P + 8) == E_NULL
    assert refused(mode=1, row_map=P) == E_NULL                 # ... a row map without the pad row is a NULL error in either mode
