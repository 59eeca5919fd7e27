"""CPU-side checks of the PLIF training entry points (sdf_plif_fwd / sdf_plif_bwd, sdf_qk_gate_plif_f32_fwd / _bwd): declared,
exported, bound, and their argument checks return before any launch (dummy device pointers, no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_plif_fwd", "sdf_plif_bwd", "sdf_plif_bwd_workspace_bytes", "sdf_qk_gate_plif_f32_fwd", "sdf_qk_gate_plif_bwd",
       "sdf_qk_gate_plif_bwd_workspace_bytes")
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def lib():
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def test_new_entry_points_are_declared_exported_and_bound(lib):
    from sdformerflow_amd import hip
    src = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|void) (sdf_\w+)\(", src, flags=re.M))
    for name in NEW:
        assert name in declared and name in hip.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.sdf_version() == 107


def test_workspace_queries_state_one_fp32_partial_per_workgroup(lib):
    # sdf_plif_bwd: one workgroup per 1024 neurons of a step; the gate: one per 256 lanes, 8 lanes per (row, head)
    assert lib.sdf_plif_bwd_workspace_bytes(C.c_int(10), C.c_int64(4096)) == 16
    assert lib.sdf_plif_bwd_workspace_bytes(C.c_int(4), C.c_int64(1028)) == 8
    assert lib.sdf_plif_bwd_workspace_bytes(C.c_int(0), C.c_int64(4096)) == 0
    assert lib.sdf_qk_gate_plif_bwd_workspace_bytes(C.c_int(2), C.c_int64(162), C.c_int(96)) == 4 * ((162 * 3 * 8 + 255) // 256)
    assert lib.sdf_qk_gate_plif_bwd_workspace_bytes(C.c_int(4), C.c_int64(32), C.c_int(192)) == 24


def test_plif_argument_errors_are_reported_before_any_launch(lib):
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)
    ws = 1 << 20

    def fwd(x=p, k=p, s=p, T=10, N=4096):
        return lib.sdf_plif_fwd(x, k, s, C.c_int(T), C.c_int64(N), C.c_float(0.1), C.c_int(1), C.c_float(0.0), None)

    assert fwd(k=None) == E_NULL and fwd(x=None) == E_NULL and fwd(s=None) == E_NULL
    assert fwd(N=4094) == E_SHAPE and fwd(N=0) == E_SHAPE
    assert fwd(x=odd) == E_ALIGN and fwd(s=odd) == E_ALIGN
    assert fwd(T=3) == E_SHAPE and fwd(T=11) == E_SHAPE

    def bwd(x=p, k=p, gs=p, gx=p, gk=p, wsp=p, wsb=ws, T=10, N=4096, surrogate=0):
        return lib.sdf_plif_bwd(x, k, gs, gx, gk, wsp, C.c_int64(wsb), C.c_int(T), C.c_int64(N), C.c_float(0.1), C.c_int(0),
                                C.c_float(0.05), C.c_int(0), C.c_int(surrogate), C.c_float(2.0), None)

    for kw in ("x", "k", "gs", "gx", "gk", "wsp"):
        assert bwd(**{kw: None}) == E_NULL, kw
    assert bwd(N=4098) == E_SHAPE
    assert bwd(T=3) == E_SHAPE and bwd(T=0) == E_SHAPE and bwd(T=40) == E_SHAPE
    assert bwd(wsb=15) == E_SHAPE                                  # needs 16 bytes at N = 4096
    assert bwd(surrogate=1) == E_DTYPE
    assert bwd(gx=odd) == E_ALIGN


def test_plif_gate_argument_errors_are_reported_before_any_launch(lib):
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def fwd(q=p, k=p, e=p, pk=p, Tq=2, rows=162, Cc=96):
        return lib.sdf_qk_gate_plif_f32_fwd(q, k, e, pk, C.c_int(Tq), C.c_int64(rows), C.c_int(Cc), C.c_float(0.1), C.c_int(1),
                                            C.c_float(0.0), None)

    assert fwd(pk=None) == E_NULL and fwd(q=None) == E_NULL
    assert fwd(Cc=48) == E_SHAPE and fwd(rows=0) == E_SHAPE and fwd(Tq=3) == E_SHAPE
    assert fwd(k=odd) == E_ALIGN

    def bwd(q=p, k=p, ge=p, gq=p, gk=p, pk=p, gpk=p, wsp=p, wsb=1 << 20, Tq=2, rows=162, Cc=96, surrogate=0):
        return lib.sdf_qk_gate_plif_bwd(q, k, ge, gq, gk, pk, gpk, wsp, C.c_int64(wsb), C.c_int(Tq), C.c_int64(rows), C.c_int(Cc),
                                        C.c_float(0.1), C.c_int(1), C.c_float(0.0), C.c_int(1), C.c_int(surrogate), C.c_float(2.0),
                                        None)

    for kw in ("q", "k", "ge", "gq", "gk", "pk", "gpk", "wsp"):
        assert bwd(**{kw: None}) == E_NULL, kw
    assert bwd(Tq=3) == E_SHAPE and bwd(Tq=8) == E_SHAPE and bwd(Cc=100) == E_SHAPE
    assert bwd(wsb=4 * ((162 * 3 * 8 + 255) // 256) - 1) == E_SHAPE
    assert bwd(surrogate=2) == E_DTYPE
    assert bwd(gq=odd) == E_ALIGN


def test_parametric_lif_node_trains_through_the_plif_function_and_keeps_its_kind():
    """Train mode reaches the HIP Function (a CPU tensor is refused by the binding, not by a NotImplementedError), the engine's
    `kind` stays "lif", and `k()` is sigmoid(w) with its graph to w."""
    import torch
    from sdformerflow_amd import hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import ParametricLIFNode
    n = ParametricLIFNode(init_tau=2.0, v_threshold=0.1, v_reset=None, detach_reset=True).train()
    assert n.kind == "lif"
    k = n.k()
    assert k.requires_grad and float(k.detach()) == 0.5
    with pytest.raises(hip.SdfError):
        n(torch.zeros(4, 8))
