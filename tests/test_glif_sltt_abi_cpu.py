"""CPU-side checks of the GLIF / SLTT-LIF training entry points (sdf_glif_fwd / sdf_glif_bwd / sdf_sltt_bwd): declared, exported,
bound, their argument checks return before any launch (dummy device pointers, no GPU needed), and the nodes reach them."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_sltt_bwd", "sdf_glif_fwd", "sdf_glif_bwd_workspace_bytes", "sdf_glif_bwd")
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


def test_glif_workspace_is_one_row_of_partials_per_workgroup(lib):
    assert lib.sdf_glif_bwd_workspace_bytes(10, 4096) == 4 * 15 * 4
    assert lib.sdf_glif_bwd_workspace_bytes(4, 3076) == 4 * 9 * 4          # four workgroups, a ragged last one
    assert lib.sdf_glif_bwd_workspace_bytes(2, 256) == 4 * 7
    assert lib.sdf_glif_bwd_workspace_bytes(3, 4096) == 0 and lib.sdf_glif_bwd_workspace_bytes(10, 0) == 0


def test_argument_errors_are_reported_before_any_launch(lib):
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def gfwd(x=p, tab=p, s=p, T=10, N=4096, dt=0):
        return lib.sdf_glif_fwd(x, tab, s, T, N, dt, None)

    assert gfwd(x=None) == E_NULL and gfwd(tab=None) == E_NULL and gfwd(s=None) == E_NULL
    for T in (0, 1, 3, 8, 16, 40):
        assert gfwd(T=T) == E_SHAPE, T
    assert gfwd(N=4094) == E_SHAPE and gfwd(N=0) == E_SHAPE
    assert gfwd(dt=2) == E_DTYPE and gfwd(x=odd) == E_ALIGN and gfwd(s=odd) == E_ALIGN

    def gbwd(x=p, tab=p, gs=p, gx=p, gt=p, wsp=p, wsb=1 << 20, T=10, N=4096, surrogate=0):
        return lib.sdf_glif_bwd(x, tab, gs, gx, gt, wsp, wsb, T, N, surrogate, 2.0, None)

    for kw in ("x", "tab", "gs", "gx", "gt", "wsp"):
        assert gbwd(**{kw: None}) == E_NULL, kw
    assert gbwd(T=3) == E_SHAPE and gbwd(T=8) == E_SHAPE and gbwd(N=4098) == E_SHAPE
    assert gbwd(surrogate=1) == E_SHAPE                               # ATan only
    assert gbwd(wsb=4 * 15 * 4 - 1) == E_SHAPE
    assert gbwd(gx=odd) == E_ALIGN

    def sbwd(x=p, gs=p, gx=p, T=10, N=4096, tau=2.0, surrogate=0):
        return lib.sdf_sltt_bwd(x, gs, gx, T, N, tau, 0.1, 1, 0.0, surrogate, 2.0, None)

    for kw in ("x", "gs", "gx"):
        assert sbwd(**{kw: None}) == E_NULL, kw
    assert sbwd(T=3) == E_SHAPE and sbwd(N=4094) == E_SHAPE and sbwd(tau=0.5) == E_SHAPE and sbwd(surrogate=1) == E_SHAPE
    assert sbwd(gs=odd) == E_ALIGN


def test_nodes_reach_the_training_functions():
    """Train mode reaches the HIP Functions: a CPU tensor is refused because there is no CPU path, not because a gradient is missing;
    the table is differentiable to all 7 + T logits."""
    from sdformerflow_amd import hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import GatedLIFNode, SLTTLIFNode
    n = GatedLIFNode(T=4).train()
    tab = n.table()
    assert tab.shape == (9,) and tab.dtype == torch.float32 and bool(((tab > 0) & (tab < 1)).all())
    tab.sum().backward()
    assert all(p.grad is not None and bool((p.grad != 0).all()) for p in n.parameters()) and len(list(n.parameters())) == 8
    with pytest.raises(NotImplementedError, match="GPU only"):
        n(torch.zeros(4, 8))
    with pytest.raises(hip.SdfError):
        n(torch.zeros(3, 8))                                          # T mismatch
    s = SLTTLIFNode(tau=2.0, v_threshold=0.1, v_reset=None).train()
    with pytest.raises(hip.SdfError):
        s(torch.zeros(4, 8, requires_grad=True))
