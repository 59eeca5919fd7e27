"""CPU-side checks of the general GLIF launch and the GLIF token gate (sdf_glif_neuron_fwd / sdf_qk_gate_glif_fwd): declared,
exported, bound, their argument checks return before any launch (dummy device pointers, no GPU needed), the ABI version is unchanged,
the host-formed gate table is the reference's expression, and the model's entry points are wired to the unfused eval plan."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_glif_neuron_fwd", "sdf_qk_gate_glif_fwd")
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
    declared = re.findall(r"^(?:int|int64_t|void) (sdf_\w+)\(", src, flags=re.M)
    for name in NEW:
        assert name in declared and name in hip.SIGNATURES, name
        assert hasattr(lib, name), name
    # each next to its sibling, in the header and in the binding's table
    for table in (declared, list(hip.SIGNATURES)):
        assert table.index("sdf_glif_neuron_fwd") == table.index("sdf_neuron_multi_fwd") + 1
        assert table.index("sdf_qk_gate_glif_fwd") == table.index("sdf_qk_gate_strided_fwd") + 1
    assert callable(hip.glif_neuron_fwd) and callable(hip.qk_gate_glif)
    assert lib.sdf_version() == 107 and "glif" not in hip.KIND              # additive: no fused entry point learns a new kind


def desc(**kw):
    """A dense (T, N) descriptor on dummy pointers, as sdf_glif_fwd's caller would lay it out."""
    from sdformerflow_amd import hip
    d = hip.NeuronDesc()
    d.x, d.out, d.T, d.out_dtype = 0x10000, 0x20000, 10, 0
    d.nb, d.ni, d.x_sb, d.x_st, d.o_sb, d.o_st = 1, 4096, 0, 4096, 0, 4096
    d.kind = 99                                                          # not read
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_general_launch_argument_errors_are_reported_before_any_launch(lib):
    p = C.c_void_p(0x30000)

    def call(tab=p, **kw):
        return lib.sdf_glif_neuron_fwd(C.byref(desc(**kw)), tab, None)

    assert lib.sdf_glif_neuron_fwd(None, p, None) == E_NULL
    assert call(tab=None) == E_NULL and call(x=None) == E_NULL and call(out=None) == E_NULL
    for T in (0, 1, 3, 8, 16, 40):                                       # 1 / 8 / 16 are legal for sdf_neuron_fwd, not here
        assert call(T=T) == E_SHAPE, T
    assert call(v_last=0x40000) == E_SHAPE
    assert call(out_dtype=7) == E_DTYPE
    assert call(x=0x10004) == E_ALIGN and call(out=0x20002, out_dtype=1) == E_ALIGN
    # sdf_neuron_fwd's own rules, in its order: shape before dtype before alignment
    assert call(ni=4098) == E_SHAPE and call(o_st=4098) == E_SHAPE and call(x_st=4098) == E_SHAPE
    assert call(ni=2, out_dtype=7) == E_SHAPE and call(out_dtype=7, x=0x10004) == E_DTYPE
    assert call(rowmap=0x50000, rowlen=6) == E_SHAPE and call(rowmap=0x50000, rowlen=96, ni=4000) == E_SHAPE
    assert call(nrep=2, rowmap=0x50000, rowlen=64) == E_SHAPE and call(nrep=2, x_srep=6) == E_SHAPE
    assert call(alpha=0x60000) == E_NULL and call(alpha=0x60000, beta=0x70000, C=6, inner=1) == E_SHAPE
    assert call(alpha=0x60004, beta=0x70000, C=8, inner=1) == E_ALIGN
    assert call(add=0x80000, add_period=6) == E_SHAPE
    assert call(tab=C.c_void_p(0x30002)) == E_ALIGN


def test_gate_argument_errors_are_reported_before_any_launch(lib):
    p, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)

    def gate(q=p, k=p, e=p, g=p, tab=p, Tq=2, rows=1000, Cc=96, ldq=None, ldk=None):
        return lib.sdf_qk_gate_glif_fwd(q, k, e, g, tab, Tq, rows, Cc, Cc if ldq is None else ldq, Cc if ldk is None else ldk, None)

    for kw in ("q", "k", "e", "tab"):
        assert gate(**{kw: None}) == E_NULL, kw
    for Tq in (0, 1, 3, 5, 10):
        assert gate(Tq=Tq) == E_SHAPE, Tq
    assert gate(Cc=48) == E_SHAPE and gate(Cc=16) == E_SHAPE and gate(rows=0) == E_SHAPE
    assert gate(ldq=96 - 16) == E_SHAPE and gate(ldk=96 - 16) == E_SHAPE and gate(ldq=104) == E_SHAPE
    assert gate(q=odd) == E_ALIGN and gate(k=odd) == E_ALIGN and gate(e=odd) == E_ALIGN


def test_host_gate_table_is_the_reference_expression():
    """The plan's tables come from a host copy of the logits with the CPU's sigmoids, the products in the reference's order: the
    expression of tests/test_glif_sltt_train_gpu.py `table_of`, on the logits of the fixture, gives the fixture's table bit for bit."""
    import numpy as np
    from sdformerflow_amd.engine_glif import gate_table
    from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import GatedLIFNode
    G = np.load(os.path.join(ROOT, "tests", "golden", "glif_grads.npz"))
    for T in (2, 4, 10):
        n = GatedLIFNode(T=T)
        n.load_state_dict({k: torch.from_numpy(G[f"T{T}/spiking_neuron.{k}"]) for k in n.state_dict()})
        assert torch.equal(gate_table(n), torch.from_numpy(G[f"T{T}_tab"])), T


def test_model_entry_points_are_wired_to_the_eval_plan():
    """Off the GPU every plan refuses to pack; what is checked is WHICH plan each entry point asks for."""
    import yaml
    from sdformerflow_amd import hip
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
    cfg = yaml.safe_load(open(os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")))
    cfg["swin_transformer"].update(input_size=[144, 144], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    made = {}
    for kind in ("glif", "lif"):
        cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
        model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy()).eval()
        for plan in (model.engine, model.eval_engine):
            with pytest.raises(hip.SdfError, match="no CPU fallback"):
                plan()
        made[kind] = model
    x = torch.zeros(1, 10, 2, 144, 144)
    for kind, model in made.items():
        def asked():
            raise LookupError("eval plan asked")
        model.eval_engine = asked
        for call in (lambda: model(x), lambda: model.forward_replicas(torch.cat([x, x]))):
            with pytest.raises(LookupError, match="eval plan asked"):
                call()
