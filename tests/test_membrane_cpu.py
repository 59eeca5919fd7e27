"""CPU-side checks of the membrane monitor's two entry points and its host arithmetic (no GPU is touched):

1. the refusal codes of sdf_neuron_vseq_fwd and sdf_membrane_stats_fwd and their order (dummy pointers: refused before any launch);
2. the reference form of the membrane the GPU tests use - `oracle.neuron_ref(x[:t+1], ..., return_aux=True)[1]`, t = 0 .. T-1 - equals,
   bit for bit, the `v_seq` of the spikingjelly stand-in's LIFNode / IFNode with `store_v_seq=True` on the same input;
3. the numpy restatement of the statistics record (monitor.membrane_record): key encoding, edge cases, and the monitor's host
   arithmetic (monitor.membrane_summary): min / max decode to the exact floats, mean = sum_q16 / 65536 / (elements - n_nan);
4. the host-side refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle.neuron_ref import neuron_ref
from sdformerflow_amd import hip
from sdformerflow_amd.monitor import (MembraneMonitor, membrane_edges, membrane_keys, membrane_record, membrane_summary, membrane_unkey)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
P = 0x10000


def loaded_lib():
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ---------------------------------------------------------------------- 1. ABI
def neuron_desc(**kw):
    d = hip.NeuronDesc()
    d.x, d.out = P, P
    d.T, d.out_dtype, d.nb, d.ni, d.x_st, d.o_st = 10, hip.SDF_U8, 1, 1028, 1028, 1028
    d.kind, d.tau, d.v_th, d.soft_reset = hip.SDF_LIF, 2.0, 0.1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_header_declares_both_entry_points_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    assert re.search(r"^int sdf_neuron_vseq_fwd\(const SdfNeuronDesc\* d, float\* v_seq, void\* stream\);", hdr, flags=re.M)
    assert re.search(r"^int sdf_membrane_stats_fwd\(const SdfMembraneStatsDesc\* d, void\* stream\);", hdr, flags=re.M)
    assert hip.SIGNATURES["sdf_neuron_vseq_fwd"] == (C.c_int, (C.POINTER(hip.NeuronDesc), C.c_void_p, C.c_void_p))
    assert hip.SIGNATURES["sdf_membrane_stats_fwd"] == (C.c_int, (C.POINTER(hip.MembraneStatsDesc), C.c_void_p))
    names = list(hip.SIGNATURES)
    assert names.index("sdf_neuron_vseq_fwd") == names.index("sdf_glif_neuron_fwd") + 1        # next to the general launches
    assert loaded_lib().sdf_version() == 107


def test_neuron_vseq_refusals_and_their_order():
    lib = loaded_lib()
    call = lambda v_seq=P, **kw: lib.sdf_neuron_vseq_fwd(C.byref(neuron_desc(**kw)), v_seq, None)
    plain = lambda **kw: lib.sdf_neuron_fwd(C.byref(neuron_desc(**kw)), None)
    assert lib.sdf_neuron_vseq_fwd(None, P, None) == E_NULL
    assert call(v_seq=None) == E_NULL
    assert call(v_seq=None, T=0) == E_NULL                          # the NULLs come first
    assert call(v_seq=P + 4) == E_ALIGN and call(v_seq=P + 8) == E_ALIGN
    assert call(kind=hip.SDF_PSN, psn_w=P, psn_b=P) == E_DTYPE      # a PSN has no membrane
    assert call(kind=hip.SDF_PSN) == E_DTYPE                        # ... refused where the kind is checked, before its pointers
    # every other check, and the order, are sdf_neuron_fwd's: the same descriptor gets the same code from both
    for kw in (dict(x=None), dict(out=None), dict(T=0), dict(ni=2), dict(out_dtype=7), dict(kind=9), dict(ni=1030), dict(o_st=1030),
               dict(x=P + 4), dict(out=P + 2), dict(nrep=2, x_srep=6), dict(rowmap=P, rowlen=6), dict(x_st=1030),
               dict(alpha=P), dict(alpha=P, beta=P, C=6, inner=1), dict(alpha=P + 4, beta=P, C=4, inner=1),
               dict(add=P, add_period=6), dict(tau=1.0), dict(v_last=P + 4),
               dict(T=0, out_dtype=7), dict(out_dtype=7, x=P + 4), dict(kind=9, ni=1030), dict(x=P + 4, tau=1.0)):
        want = plain(**kw)
        assert want < 0 and call(**kw) == want, kw
    assert call(out_dtype=7, kind=hip.SDF_PSN) == E_DTYPE and call(T=0, kind=hip.SDF_PSN) == E_SHAPE     # shape, then dtype and kind
    assert call(kind=hip.SDF_PSN, x=P + 4) == E_DTYPE               # the kind before the alignment
    assert call(v_seq=P + 4, tau=1.0) == E_SHAPE                    # v_seq's alignment behind the descriptor's own checks


def stats_desc(**kw):
    d = hip.MembraneStatsDesc()
    d.v, d.table = P, 0x20000
    d.outer, d.T, d.rows, d.C, d.row_stride, d.bins = 1, 10, 7, 17, 17, 64
    d.lo, d.hi, d.inv_width = hip.membrane_inv_width(-0.2, 0.2, 64)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_membrane_stats_refusals_and_their_order():
    lib = loaded_lib()
    call = lambda **kw: lib.sdf_membrane_stats_fwd(C.byref(stats_desc(**kw)), None)
    assert lib.sdf_membrane_stats_fwd(None, None) == E_NULL
    assert call(v=None) == E_NULL and call(table=None) == E_NULL
    for field in ("outer", "rows", "C"):
        assert call(**{field: 0}) == E_SHAPE and call(**{field: -3}) == E_SHAPE, field
    assert call(T=0) == E_SHAPE and call(T=65) == E_SHAPE
    assert call(row_stride=16) == E_SHAPE                           # row_stride < C
    assert call(bins=0) == E_SHAPE and call(bins=257) == E_SHAPE
    assert call(hi=-0.2) == E_SHAPE and call(hi=-0.3) == E_SHAPE    # hi <= lo
    assert call(lo=float("nan")) == E_SHAPE
    assert call(inv_width=0.0) == E_SHAPE and call(inv_width=float("inf")) == E_SHAPE
    assert call(v=P + 2) == E_ALIGN and call(table=0x20004) == E_ALIGN
    assert call(v=None, T=0) == E_NULL and call(T=0, table=0x20004) == E_SHAPE and call(bins=0, v=P + 2) == E_SHAPE
    assert call(outer=1 << 40) == E_SHAPE and call(rows=1 << 59) == E_SHAPE


def test_bindings_refuse_on_the_host():
    with pytest.raises(hip.SdfError, match="device tensor"):
        hip.membrane_stats(torch.zeros((10, 4, 8)), 0)
    with pytest.raises(hip.SdfError):
        hip.membrane_stats([[0.0]], 0)
    lo, hi, inv = hip.membrane_inv_width(-0.2, 0.2, 64)
    assert (lo, hi) == (float(np.float32(-0.2)), float(np.float32(0.2))) and inv == float(np.float32(64) / (np.float32(0.2) - np.float32(-0.2)))


# ---------------------------------------------------------------------- 2. the reference form of the membrane
@pytest.fixture
def sj_neuron():
    """The spikingjelly stand-in's neuron module (oracle/stubs), imported without leaving it on sys.path or in sys.modules."""
    stubs = os.path.join(ROOT, "oracle", "stubs")
    before = set(sys.modules)
    sys.path.insert(0, stubs)
    try:
        from spikingjelly.activation_based import neuron
        yield neuron
    finally:
        sys.path.remove(stubs)
        for m in set(sys.modules) - before:
            if m == "spikingjelly" or m.startswith("spikingjelly."):
                del sys.modules[m]


@pytest.mark.parametrize("kind,tau,v_reset", [("lif", 2.0, None), ("lif", 2.0, 0.0), ("lif", 3.0, None), ("lif", 3.0, -0.05),
                                              ("lif", 1.7, 0.02), ("if", 2.0, None), ("if", 2.0, 0.0)])
def test_prefix_reference_is_spikingjellys_v_seq(sj_neuron, kind, tau, v_reset):
    """Soft and hard reset, tau 2 and taus that are no power of two, T = 4."""
    T, v_th = 4, 0.1
    g = torch.Generator().manual_seed(int(tau * 10) + (0 if v_reset is None else 1))
    x = torch.rand((T, 3, 1031), generator=g) * 0.9 - 0.3
    heaviside = lambda u: (u >= 0).to(u.dtype)
    node = (sj_neuron.IFNode(v_threshold=v_th, v_reset=v_reset, surrogate_function=heaviside, store_v_seq=True) if kind == "if" else
            sj_neuron.LIFNode(tau=tau, v_threshold=v_th, v_reset=v_reset, surrogate_function=heaviside, store_v_seq=True))
    with torch.no_grad():
        s_sj = node.multi_step_forward(x)
    runs = [neuron_ref(x[:t + 1], kind, tau, v_th, v_reset, return_aux=True) for t in range(T)]
    v_ref = torch.stack([v for _, v in runs])
    assert torch.equal(runs[-1][0], s_sj) and 0 < int(s_sj.sum()) < s_sj.numel()
    assert all(torch.equal(runs[t][0], s_sj[:t + 1]) for t in range(T))
    assert v_ref.shape == node.v_seq.shape and torch.equal(v_ref.view(torch.int32), node.v_seq.view(torch.int32))


# ---------------------------------------------------------------------- 3. the record and the host arithmetic
def test_key_encoding_orders_floats_and_decodes_exactly():
    vals = np.array([-np.inf, -3.5, -1e-41, -0.0, 0.0, 1e-41, 1e-20, 0.1, 3.5, np.inf], dtype=np.float32)
    keys = membrane_keys(vals)
    assert keys.dtype == np.int64 and (np.diff(keys) > 0).all() and keys.min() > 0 and keys.max() < 0xFFFFFFFF
    assert keys[3] == 0x7FFFFFFF and keys[4] == 0x80000000            # -0 sorts directly below +0
    back = membrane_unkey(keys)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), vals.view(np.uint32))
    rng = np.random.default_rng(0)
    r = rng.standard_normal(10000).astype(np.float32) * 1e3
    assert np.array_equal(np.argsort(membrane_keys(r), kind="stable"), np.argsort(r, kind="stable"))
    assert np.array_equal(membrane_unkey(membrane_keys(r)), r)


def test_record_edge_cases():
    lo, hi, bins = -0.2, 0.2, 4                                       # inner edges at -0.1, 0, 0.1 (as fp32 arithmetic places them)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    row = np.array([0.0, -0.0, 1e-41, np.inf, -np.inf, np.nan, lo32, hi32, np.nextafter(lo32, np.float32(-1)), np.nextafter(hi32, np.float32(0)),
                    0.5 / 65536, 1.5 / 65536, 2.5 / 65536, -0.5 / 65536, 40000.0, -40000.0], dtype=np.float32)
    rec = membrane_record(row[None], lo, hi, bins)[0]
    assert rec.shape == (4 + bins + 2,) and rec[0] == 1
    # ties of rintf go to even; beyond +-32768 the sum takes the clamp, +-inf included: they cancel here
    near = sum(int(np.rint(x * np.float32(65536))) for x in row[6:10])            # lo, hi and their neighbours: no ties
    assert rec[1] == near + (0 + 2 + 2 - 0) + (2 ** 31 - 2 ** 31) * 2               # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0
    assert membrane_unkey(rec[2]) == -np.inf and membrane_unkey(rec[3]) == np.inf
    hist = rec[4:]
    assert hist.sum() == row.size - 1                                 # every number lands in exactly one slot, the NaN in none
    assert hist[0] == 3                                               # -inf, just below lo, -40000
    assert hist[bins + 1] == 3                                        # +inf, hi itself, 40000
    assert hist[1] == 1                                               # lo itself opens the first bin
    assert hist[bins] == 1                                            # just below hi: the last bin (the min() clamp holds it there)
    assert hist[2] == 1 and hist[3] == 6                              # -0.5 / 65536 below the edge at 0; +-0, the denormal and the ties on it
    # -0.0 and 0.0 are equal numbers: both give (0 - lo) * inv_width; only their keys differ
    both = membrane_record(np.array([[0.0, -0.0]], dtype=np.float32), lo, hi, bins)[0]
    assert both[4:].max() == 2 and both[2] == 0x7FFFFFFF and both[3] == 0x80000000
    # an all-NaN step: counted, nothing else moves
    nan = membrane_record(np.full((1, 5), np.nan, dtype=np.float32), lo, hi, bins)[0]
    assert nan[0] == 5 and nan[1] == 0 and nan[2] == 0xFFFFFFFF and nan[3] == 0 and nan[4:].sum() == 0


def test_histogram_index_is_the_fp32_formula():
    """Element by element against the formula written out with separately rounded fp32 operations."""
    lo, hi, bins = -0.2, 0.2, 64
    lo32, hi32, inv = (np.float32(a) for a in hip.membrane_inv_width(lo, hi, bins))
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.uniform(-0.3, 0.3, 5000), membrane_edges(lo, hi, bins)]).astype(np.float32)
    hist = np.zeros(bins + 2, dtype=np.int64)
    for x in v:
        i = 0 if x < lo32 else bins + 1 if x >= hi32 else 1 + min(bins - 1, int(np.floor(np.float32(np.float32(x - lo32) * inv))))
        hist[i] += 1
    assert np.array_equal(membrane_record(v[None], lo, hi, bins)[0, 4:], hist)
    edges = membrane_edges(lo, hi, bins)
    assert edges.dtype == np.float64 and edges.shape == (bins + 1,) and edges[0] == float(lo32) and edges[-1] == float(hi32)


def test_host_arithmetic_of_the_monitor():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal((2, 10, 3000)) * 0.2).astype(np.float32)            # two forwards
    a[0, 3, 5] = np.nan
    a[1, 7, :] = np.nan                                                           # a step without a number in one forward
    recs = np.stack([membrane_record(f, -0.2, 0.2, 16) for f in a])
    s = membrane_summary(recs, 3000)
    assert s["n_nan"].tolist() == [0, 0, 0, 1, 0, 0, 0, 3000, 0, 0]
    flat = np.moveaxis(a, 1, 0).reshape(10, -1)
    assert np.array_equal(s["min"], np.nanmin(flat, 1).astype(np.float64)) and np.array_equal(s["max"], np.nanmax(flat, 1).astype(np.float64))
    assert np.array_equal(s["mean"], recs[:, :, 1].sum(0) / 65536 / (2 * 3000 - s["n_nan"]))
    assert np.abs(s["mean"] - np.nanmean(flat.astype(np.float64), 1)).max() <= 2.0 ** -17
    assert s["hist"].shape == (10, 18) and np.array_equal(s["hist"].sum(1), 2 * 3000 - s["n_nan"])
    empty = membrane_summary(membrane_record(np.full((1, 4), np.nan, dtype=np.float32), -1, 1, 4)[None], 4)
    assert np.isnan(empty["mean"][0]) and np.isnan(empty["min"][0]) and np.isnan(empty["max"][0])


# ---------------------------------------------------------------------- 4. host-side refusals
def test_monitor_refuses_what_it_cannot_record():
    from sdformerflow_amd.STSwinNet.STSwinNet import STTFlowNet
    from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    with pytest.raises(hip.SdfError, match="spiking model"):
        MembraneMonitor(STTFlowNet.__new__(STTFlowNet))
    with pytest.raises(hip.SdfError, match="SEW family"):
        MembraneMonitor(SpikingformerFlowNet.__new__(SpikingformerFlowNet))
    with pytest.raises(hip.SdfError, match="GLIF node has no v_seq"):
        hip.neuron_fwd(None, None, 4, 1, 8, 0, 8, 0, 8, hip.GlifParams(None), v_seq=torch.zeros(1))
