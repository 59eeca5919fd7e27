"""Host side of the streamed evaluation, no GPU: FlowMetrics.result()'s arithmetic on a hand-filled table, the new entry points in the
header and in the binding's signature table, their argument checks (refused before any launch), and the evaluator's dealing of
samples to streams and groups."""
import ctypes as C
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdf_flow_metrics_workspace_bytes", "sdf_flow_metrics_fwd", "sdf_prepare_chunk_workspace_bytes", "sdf_prepare_chunk_fwd")


def test_result_arithmetic_on_a_hand_filled_table():
    from sdformerflow_amd.loss.flow_supervised import FlowMetrics
    m = FlowMetrics(4, device="cpu")
    # {n_valid, sum_err, n_pe1, n_pe2, n_pe3, n_outlier, sum_ang, n_pixels}
    m.table[0] = torch.tensor([100.0, 250.0, 60.0, 40.0, 20.0, 10.0, 50.0, 128.0], dtype=torch.float64)
    m.table[1] = torch.tensor([50.0, 25.0, 5.0, 0.0, 0.0, 0.0, 100.0, 128.0], dtype=torch.float64)
    m.table[2] = torch.tensor([7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0, 128.0], dtype=torch.float64)      # (beyond n: not a sample yet)
    m.n = 2
    assert m.counts().shape == (2, 8)
    r = m.result()
    assert set(r) == {"AEE", "PE1", "PE2", "PE3", "outliers", "AAE"}
    assert r["AEE"] == (250.0 / (100.0 + 1e-9) + 25.0 / (50.0 + 1e-9)) / 2
    assert r["PE1"] == (60.0 / (100.0 + 1e-9) + 5.0 / (50.0 + 1e-9)) / 2
    assert r["PE2"] == (40.0 / (100.0 + 1e-9)) / 2 and r["PE3"] == (20.0 / (100.0 + 1e-9)) / 2
    assert r["outliers"] == (10.0 / (100.0 + 1e-9)) / 2
    assert r["AAE"] == (50.0 / 100.0 * 180 / math.pi + 100.0 / 50.0 * 180 / math.pi) / 2
    assert set(m.result(("AEE",))) == {"AEE", "PE1", "PE2", "PE3", "outliers"} and set(m.result(("AAE",))) == {"AAE"}
    with pytest.raises(ValueError):
        m.result(("EPE",))
    # a sample without a valid pixel: AEE 0 (the class's n + 1e-9), AAE NaN (the class's 0 / 0)
    m.table[2] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 128.0], dtype=torch.float64)
    m.n = 3
    r3 = m.result()
    assert r3["AEE"] == (250.0 / (100.0 + 1e-9) + 25.0 / (50.0 + 1e-9) + 0.0) / 3 and math.isnan(r3["AAE"])
    # no sample at all: zeros, as the loops' max(it, 1)
    assert FlowMetrics(2, device="cpu").result(("AEE",)) == {"AEE": 0.0, "PE1": 0.0, "PE2": 0.0, "PE3": 0.0, "outliers": 0.0}
    # a larger table takes the records over
    m.reserve(10)
    assert m.table.shape == (10, 8) and m.result()["PE1"] == r3["PE1"] and not m.table[3:].any()


def test_new_entry_points_are_declared_and_bound():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    assert "typedef struct SdfFlowMetricsDesc" in hdr and "typedef struct SdfPrepareChunkDesc" in hdr
    assert hip.SIGNATURES["sdf_flow_metrics_fwd"] == (C.c_int, (C.POINTER(hip.FlowMetricsDesc), C.c_void_p))
    assert hip.SIGNATURES["sdf_prepare_chunk_fwd"] == (C.c_int, (C.POINTER(hip.PrepareChunkDesc), C.c_void_p))
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107         # (additive exports: the version stays)
    build = open(os.path.join(ROOT, "sdformerflow_amd", "csrc", "build.sh")).read()
    assert " flow_metrics " in build and " prepare_chunk;" in build


def test_argument_errors_of_the_new_entry_points():
    """Dummy pointers: every refusal comes before any launch, so this needs no GPU."""
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = hip.lib()
    p = 0x10000
    assert lib.sdf_flow_metrics_workspace_bytes(1, 288, 384) == 108 * 8 * 8          # one partial record per 1024 pixels
    assert lib.sdf_flow_metrics_workspace_bytes(3, 37, 53) == 3 * 2 * 8 * 8
    assert lib.sdf_flow_metrics_workspace_bytes(0, 4, 4) == 0 and lib.sdf_flow_metrics_workspace_bytes(1, 1 << 15, 1 << 15) == 0
    assert lib.sdf_flow_metrics_fwd(None, None) == hip.E_NULL

    def fm(**kw):
        d = hip.FlowMetricsDesc()
        d.pred = d.label = d.valid = d.table = d.workspace = p
        d.workspace_bytes, d.B, d.H, d.W, d.row0, d.rows, d.flow_scaling = 1 << 20, 2, 37, 53, 0, 2, 1.0
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sdf_flow_metrics_fwd(C.byref(d), None)
    assert fm(pred=None) == hip.E_NULL and fm(table=None) == hip.E_NULL and fm(workspace=None) == hip.E_NULL
    assert fm(B=0) == hip.E_SHAPE and fm(W=0) == hip.E_SHAPE
    assert fm(row0=1) == hip.E_SHAPE and fm(row0=-1) == hip.E_SHAPE and fm(rows=1) == hip.E_SHAPE      # rows outside the table
    assert fm(workspace_bytes=2 * 2 * 64 - 1) == hip.E_SHAPE
    assert fm(label=p + 2) == hip.E_ALIGN and fm(table=p + 4) == hip.E_ALIGN and fm(event_mask=p + 1) == hip.E_ALIGN

    assert lib.sdf_prepare_chunk_workspace_bytes(3) == 24 and lib.sdf_prepare_chunk_workspace_bytes(0) == 0
    assert lib.sdf_prepare_chunk_fwd(None, None) == hip.E_NULL

    def pc(**kw):
        d = hip.PrepareChunkDesc()
        d.voxel = d.out = d.workspace = p
        d.workspace_bytes, d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.crop_oy, d.crop_ox, d.norm = 256, 3, 2, 9, 11, 6, 8, 1, 1, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sdf_prepare_chunk_fwd(C.byref(d), None)
    assert pc(voxel=None) == hip.E_NULL and pc(out=None) == hip.E_NULL and pc(workspace=None) == hip.E_NULL
    assert pc(norm=2) == hip.E_DTYPE and pc(norm=-1) == hip.E_DTYPE                 # "std" is the torch function's
    assert pc(crop_oy=4) == hip.E_SHAPE and pc(crop_ox=4) == hip.E_SHAPE            # the window leaves the volume
    assert pc(crop_h=0) == hip.E_SHAPE and pc(crop_h=0, crop_w=0) == hip.E_SHAPE    # half a crop; an origin without a crop
    assert pc(B=0) == hip.E_SHAPE and pc(bins=0) == hip.E_SHAPE
    assert pc(workspace_bytes=23) == hip.E_SHAPE
    assert pc(out=p + 2) == hip.E_ALIGN and pc(event_mask=p + 2) == hip.E_ALIGN and pc(workspace=p + 4) == hip.E_ALIGN


def test_wrappers_refuse_cpu_tensors():
    from sdformerflow_amd import hip
    z = torch.zeros(1, 2, 4, 4)
    with pytest.raises(hip.SdfError):
        hip.flow_metrics(z, z, torch.ones(1, 4, 4))
    with pytest.raises(hip.SdfError):
        hip.prepare_chunk(torch.zeros(1, 2, 4, 4))


@pytest.mark.parametrize("streams,replicas", [(1, 1), (1, 4), (2, 3), (2, 10), (3, 2), (4, 7)])
def test_dealing_covers_every_sample_exactly_once(streams, replicas):
    from sdformerflow_amd import harness
    for n in range(26):
        plan = harness.stream_plan(n, streams, replicas)
        assert [i for _, k, m in plan for i in range(k, k + m)] == list(range(n))           # each once, numbered in iteration order
        assert all(1 <= m <= replicas for _, _, m in plan) and all(m == replicas for _, _, m in plan[:-1])
        assert [j for j, _, _ in plan] == [g % streams for g in range(len(plan))]            # groups go round-robin
        dealt = list(harness.deal(iter("abcdefghijklmnopqrstuvwxyz"[:n]), streams, replicas))
        assert [(j, k, len(g)) for j, k, g in dealt] == plan and "".join(c for _, _, g in dealt for c in g) == "abcdefghijklmnopqrstuvwxyz"[:n]
