"""Host side of the stage-0, head and tail entry points (csrc/head_tail.hip, pred_head.hip, spike_gemm.hip on 16-bit planes, qk_gate.hip,
qk_attn.hip, elementwise.hip's layer norm, win_attn.hip), pinned without a GPU before their neuron check and their template dispatch
were stated once (csrc/host_launch.h): the return code of calls that are REFUSED BEFORE ANY LAUNCH.

  * one broken argument at a time, in the order of each entry point's checks;
  * where an entry point takes a neuron: the three neuron faults - an unknown kind, PSN without its pointers, LIF with tau = 1 - alone
    and each crossed with faults the entry point checks BEFORE the neuron (their code wins) and AFTER it (the neuron's code wins), so the
    place of the neuron check among the others is pinned, not only its codes.  sdf_qk_attn_fwd and sdf_ms_mlp_fwd have no neuron check
    of their own: a fault in their first neuron is refused by the first step of the three-launch form (sdf_neuron_fwd), where the
    operand's alignment stands between the kind and the other two clauses.

Dummy aligned pointers do: nothing is dereferenced on the way to a refusal.  The expected codes are those of the library before the
refactor: `SDF_HIP_LIB=<a build of that commit> python tests/test_stage0_host_cpu.py` writes tests/golden/stage0_host_codes.json.  The
file skips itself where a GPU is present: a regression that turned a refusal into a launch must not run a kernel on dummy pointers."""
import ctypes as C
import copy
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage0_host_codes.json")
P, P2, ODD16, ODD4, ODD256 = 0x10000, 0x20000, 0x10004, 0x10002, 0x10010     # aligned; another; not 16- / 4- / 256-byte aligned
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
LIF, PSN, IF = 0, 1, 2
ANN, SEW = 0, 1                                   # SDF_ATTN_ANN, SDF_ATTN_SEW

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-only pins on dummy pointers: never beside a GPU")


@pytest.fixture(scope="module")
def lib():
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """The answers are those of the default routing: no SDF_* tuning switch (SDF_HIP_LIB names the library and stays)."""
    for name in [n for n in os.environ if n.startswith("SDF_") and n != "SDF_HIP_LIB"]:
        monkeypatch.delenv(name)


def fill(d, **kw):
    for f, v in kw.items():
        if isinstance(v, dict):
            fill(getattr(d, f), **v)
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                getattr(d, f)[i] = e
        else:
            setattr(d, f, v)
    return d


def merged(a, b):
    """b over a, one level into nested dicts (the g of a convolution, a neuron)"""
    out = dict(a)
    for k, v in b.items():
        out[k] = merged(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def crossed(neuron_faults, before, after):
    """every neuron fault with every fault checked before it and every fault checked after it"""
    return [merged(n, o) for n in neuron_faults for o in before + after]


# the three neuron faults as (kind, tau, psn_w, psn_b) over a valid LIF
GOOD = dict(kind=LIF, tau=2.0, v_th=0.1, v_reset=0.0, soft_reset=1)
FAULTS = [dict(kind=3), dict(kind=PSN), dict(tau=1.0)]
PSN_OK = dict(kind=PSN, psn_w=P, psn_b=P)


def flat(prefix):
    """the faults on a descriptor that carries the neuron as plain fields (`sn_kind` or `kind`, tau, psn_w, psn_b)"""
    return [{(prefix if k == "kind" else k): v for k, v in f.items()} for f in FAULTS]


def nested(*fields):
    """... as SdfNeuronCfg members"""
    return [{f: dict(v) for f in fields} for v in FAULTS]


# ------------------------------------------------------------------------------------------------------------ sdf_head_conv_sn_fwd
def head_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(x=P, w=P, out=P, B=1, T=10, H=2, W=32, Cin=2, Cout=48, sn_kind=LIF, tau=2.0, v_th=0.1, soft_reset=1)
    return fill(hip.HeadConvDesc(), **merged(base, kw))


HEAD = [
    dict(x=None), dict(w=None), dict(out=None), dict(B=0), dict(H=0), dict(W=0), dict(W=24), dict(alpha=P), *flat("sn_kind"), dict(out=ODD16),
    dict(B=65536, H=65536, W=16),                                                     # more tiles than a grid holds
    dict(T=7), dict(T=7, W=16), dict(Cout=40), dict(Cout=40, W=16), dict(Cin=4, Cout=32), dict(Cin=3),      # no kernel: after every check
    dict(sn_kind=PSN, psn_w=P, psn_b=P, T=7),
    dict(x=None, B=0), dict(B=0, alpha=P), dict(T=7, out=ODD16),
    *crossed(flat("sn_kind"), [dict(alpha=P), dict(W=24)], [dict(out=ODD16), dict(T=7)]),
]


# ------------------------------------------------------------------------------------------------------------ sdf_pred_head_fwd
def pred_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(z=P, wgt=P, pred=P, B=1, D=10, h=2, w=4, Cin=96, sn_pred=GOOD, sn_next=GOOD)
    return fill(hip.PredHeadDesc(), **merged(base, kw))


NEXT = dict(next_spikes=P, next_ld=128, next_z_off=0, next_pred_off=96, next_zero_off=100, next_zero_len=28)
PRED = [
    dict(z=None), dict(wgt=None), dict(pred=None), dict(B=0), dict(h=0), dict(w=0), dict(Cin=100), dict(Cin=48), dict(D=7), dict(D=0),
    *nested("sn_pred"), dict(sn_pred=PSN_OK, D=20), dict(pred=None, flow=P, H=3, W=8), dict(pred=None, flow=P, H=4, W=6), dict(flow=P, H=1, W=8),
    *[merged(NEXT, f) for f in nested("sn_next")], dict(NEXT, sn_next=PSN_OK), dict(NEXT, sn_next=dict(soft_reset=0)),
    dict(NEXT, next_ld=0), dict(NEXT, next_ld=126), dict(NEXT, next_z_off=64), dict(NEXT, next_pred_off=126), dict(NEXT, next_zero_len=32),
    dict(NEXT, next_spikes=ODD4), dict(z=ODD16), dict(wgt=ODD16), dict(pred=ODD16), dict(keep_spikes=ODD4),
    dict(B=65536, h=65536, w=16),                                                     # more workgroups than a grid holds
    dict(z=None, B=0), dict(B=0, Cin=100), dict(D=7, z=ODD16),
    *crossed(nested("sn_pred"), [dict(D=7), dict(pred=None)], [dict(z=ODD16), dict(flow=P, H=3, W=8)]),
    *[merged(NEXT, v) for v in crossed(nested("sn_next"), [dict(flow=P, H=3, W=8), dict(sn_pred=dict(kind=3))], [dict(next_ld=0), dict(next_spikes=ODD4)])],
]


# ------------------------------------------------------------------------------------- sdf_spike_gemm_fwd, 16-bit planes (streaming kernel)
def gemm_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(A=P, Wp=P, out=P, M=1080, N=96, K=128, lda=128, ldo=96, nsplit=2, acc_scale=1.0)
    return fill(hip.SpikeGemmDesc(), **merged(base, kw))


SPIKE = dict(sn_T=10, sn_kind=LIF, tau=2.0, v_th=0.1, soft_reset=1, out_spike=P, pos_count=108, pos_inner=108, t_stride=108)
ZG = dict(zg_nH=4, zg_T=2, zg_B=5, zg_N1=108)
GEMM = [
    dict(A=None), dict(Wp=None), dict(out=None), dict(SPIKE, out_spike=None), dict(M=0), dict(M=1 << 31), dict(N=16), dict(N=48), dict(K=16),
    dict(K=48, lda=48), dict(nsplit=0), dict(nsplit=7), dict(acc_scale=3.0), dict(acc_scale=0.0), dict(nsplit=1, acc_scale=2.0),
    dict(nsplit=3, acc_scale=0.5), dict(alpha=P), dict(lda=136),
    dict(SPIKE, pos_count=100), dict(SPIKE, pos_inner=0), *[merged(SPIKE, f) for f in flat("sn_kind")], dict(SPIKE, add=P),
    dict(SPIKE, zg_nH=4), dict(SPIKE, out_rowmap=P), dict(SPIKE, resid=P), dict(SPIKE, bias=P), dict(SPIKE, out_spike=ODD16),
    dict(ZG, K=96, lda=96), dict(ZG, zg_T=0), dict(ZG, zg_B=4), dict(ZG, zg_rep=-1), dict(ZG, zg_rep=3), dict(A=ODD16), dict(Wp=ODD16),
    dict(ldo=98), dict(out=ODD16), dict(resid=ODD16), dict(bias=ODD16), dict(alpha=ODD16, beta=P), dict(alpha=P, beta=ODD16),
    dict(SPIKE, sn_T=7, M=756), dict(SPIKE, sn_T=3, M=324), dict(SPIKE, sn_T=7, M=756, nsplit=1), dict(SPIKE, sn_T=7, M=756, nsplit=3, N=64),
    dict(A=None, M=0), dict(M=0, nsplit=0), dict(nsplit=0, alpha=P), dict(alpha=P, lda=136), dict(lda=136, A=ODD16),
    *[merged(SPIKE, v) for v in crossed(flat("sn_kind"), [dict(alpha=P), dict(pos_count=100)], [dict(out_spike=ODD16), dict(add=P), dict(bias=P)])],
]


# ------------------------------------------------------------------------------------- sdf_spike_conv2d_fwd, 16-bit planes
def conv_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(H=12, W=12, Cin=128, OH=12, OW=12, KH=3, KW=3, sy=1, sx=1, dy=(-1, 0, 1), dx=(-1, 0, 1),
                g=dict(A=P, Wp=P, out=P, M=1440, N=64, K=1152, ldo=64, nsplit=2, acc_scale=1.0))
    return fill(hip.SpikeConvDesc(), **merged(base, kw))


CSPIKE = dict(sn_T=10, sn_kind=LIF, tau=2.0, v_th=0.1, soft_reset=1, out_spike=P, pos_count=144, pos_inner=144, pos_ostride=1440, t_stride=144)
CONV = [
    dict(g=dict(A=None)), dict(g=dict(Wp=None)), dict(g=dict(out=None)), dict(g=dict(CSPIKE, out_spike=None)), dict(H=0), dict(W=40000),
    dict(OH=0), dict(Cin=32, g=dict(K=288)), dict(Cin=72, g=dict(K=648)), dict(KH=4), dict(KW=0), dict(sy=0), dict(g=dict(K=1024)),
    dict(g=dict(N=48)), dict(g=dict(M=1441)), dict(g=dict(nsplit=0)), dict(g=dict(nsplit=6)), dict(g=dict(acc_scale=3.0)),
    dict(g=dict(nsplit=1, acc_scale=2.0)), dict(g=dict(alpha=P)), dict(g=dict(zg_nH=4)),
    dict(g=dict(CSPIKE, sn_T=7)), dict(g=dict(CSPIKE, sn_T=5, pos_count=288)), dict(g=dict(CSPIKE, sn_T=20, pos_count=72)), dict(g=dict(CSPIKE, pos_count=100)),
    dict(g=dict(CSPIKE, pos_inner=0)), *[dict(g=merged(CSPIKE, f)) for f in flat("sn_kind")], dict(g=dict(CSPIKE, out_rowmap=P)),
    dict(g=dict(CSPIKE, bias=P)), dict(g=dict(CSPIKE, add=P)), dict(g=dict(CSPIKE, out=None, resid=P)), dict(g=dict(CSPIKE, ldo=32)),
    dict(g=dict(CSPIKE, out=ODD4)), dict(g=dict(CSPIKE, out_spike=ODD16)), dict(g=dict(A=ODD16)), dict(g=dict(Wp=ODD16)),
    dict(g=dict(A=None), H=0), dict(H=0, g=dict(nsplit=0)), dict(g=dict(nsplit=0, alpha=P)), dict(g=dict(alpha=P, zg_nH=4)), dict(g=dict(zg_nH=4, A=ODD16)),
    *[dict(g=merged(CSPIKE, v)) for v in crossed(flat("sn_kind"), [dict(alpha=P), dict(pos_count=100)], [dict(out_spike=ODD16), dict(bias=P), dict(out=None, resid=P)])],
]


# ------------------------------------------------------------------------------------- sdf_qk_gate_fwd / sdf_qk_gate_strided_fwd
def gate_args(strided, **kw):
    a = merged(dict(q=P, k=P2, e=P, Tq=2, rows=10, C=64, ldq=64, ldk=64, kind=LIF, tau=2.0, v_th=0.1, v_reset=0.0, soft_reset=1,
                    psn_w=None, psn_b=None), kw)
    names = ["q", "k", "e", "Tq", "rows", "C"] + (["ldq", "ldk"] if strided else []) + ["kind", "tau", "v_th", "v_reset", "soft_reset", "psn_w", "psn_b"]
    return [a[n] for n in names] + [None]


GATE = [
    dict(q=None), dict(k=None), dict(e=None), dict(Tq=0), dict(Tq=5), dict(rows=0), dict(C=16), dict(C=48), *flat("kind"),
    dict(kind=PSN, psn_w=P), dict(q=ODD16), dict(k=ODD16), dict(e=ODD16), dict(q=None, Tq=0), dict(Tq=0, kind=3),
    *crossed(flat("kind"), [dict(q=None), dict(C=48)], [dict(e=ODD16)]),
]
GATE_STRIDED = GATE + [
    dict(ldq=32), dict(ldk=32), dict(ldq=72), dict(ldk=72), dict(C=48, ldq=72), *crossed(flat("kind"), [dict(ldq=32), dict(ldk=72)], [dict(q=ODD16)]),
]


# ------------------------------------------------------------------------------------- sdf_qk_attn_fwd
def attn_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(x=P, slice_map=P, B_=4, x_rows=200, Tq=2, N1=25, C=96, nH=3, nsplit=2, q_planes=P, k_planes=P, p_planes=P,
                q_acc_scale=1.0, k_acc_scale=1.0, p_acc_scale=1.0, sn_proj=GOOD, sn_q=GOOD, sn_k=GOOD, sn2_q=GOOD, workspace=P,
                workspace_bytes=1 << 40)
    return fill(hip.QkAttnDesc(), **merged(base, kw))


ATTN_SN = ("sn_proj", "sn_q", "sn_k", "sn2_q")
ATTN = [
    dict(x=None), dict(slice_map=None), dict(workspace=None), dict(p_planes=None), dict(q_planes=None), dict(k_planes=None),
    dict(B_=0), dict(Tq=0), dict(N1=0), dict(C=16), dict(C=48), dict(nH=0), dict(nH=2), dict(workspace_bytes=1000), dict(rep_windows=-1),
    dict(rep_windows=3), dict(workspace=ODD256), dict(emit_s1=P),
    *nested(*ATTN_SN), *nested("sn_proj"), dict(x=ODD16),            # (the first neuron refuses; x's alignment is sdf_neuron_fwd's check)
    dict(x=None, B_=0), dict(B_=0, workspace=ODD256), dict(workspace=ODD256, emit_s1=P),
    *crossed(nested(*ATTN_SN), [dict(workspace_bytes=1000), dict(workspace=ODD256), dict(emit_s1=P)], [dict(x=ODD16)]),
]


# ------------------------------------------------------------------------------------- sdf_ms_mlp_fwd
def mlp_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(x=P, B=1, D=10, HW=63, C=96, Ch=384, nsplit=2, fc1_planes=P, fc2_planes=P, fc1_alpha=P, fc1_beta=P, fc2_alpha=P,
                fc2_beta=P, fc1_acc_scale=1.0, fc2_acc_scale=1.0, sn1=GOOD, sn2=GOOD, workspace=P, workspace_bytes=1 << 40)
    return fill(hip.MsMlpDesc(), **merged(base, kw))


MLP = [
    dict(x=None), dict(fc1_planes=None), dict(fc2_planes=None), dict(workspace=None), dict(B=0), dict(D=0), dict(HW=0), dict(C=16), dict(C=48),
    dict(Ch=16), dict(Ch=400), dict(workspace_bytes=1000), dict(workspace=ODD256), dict(s1_in=P), dict(emit_next=P),
    *nested("sn1", "sn2"), *nested("sn1"), dict(x=ODD16),
    dict(x=None, B=0), dict(B=0, workspace=ODD256), dict(workspace=ODD256, s1_in=P),
    *crossed(nested("sn1", "sn2"), [dict(workspace_bytes=1000), dict(workspace=ODD256), dict(s1_in=P)], [dict(x=ODD16)]),
    *[merged(dict(C=192, Ch=768, D=d), f) for d in (5, 20) for f in nested("sn1", "sn2")],
]


# ------------------------------------------------------------------------------------- sdf_layer_norm_fwd
def ln_args(**kw):
    a = merged(dict(x=P, gamma=P, beta=P, out=P, rows=3, C=96, eps=1e-5), kw)
    return [a[n] for n in ("x", "gamma", "beta", "out", "rows", "C", "eps")] + [None]


LN = [
    dict(x=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(C=0), dict(C=6), dict(C=2052),
    dict(C=4096), dict(x=ODD16), dict(gamma=ODD16), dict(beta=ODD16), dict(out=ODD16), dict(x=None, rows=0), dict(rows=0, x=ODD16),
    dict(C=6, out=ODD16),
]


# ------------------------------------------------------------------------------------- sdf_win_attn_fwd
def win_desc(**kw):
    from sdformerflow_amd import hip
    base = dict(mode=ANN, q=P, k=P, v=P, out=P, B_=4, nW=1, nH=3, N=128, hd=32, scale=P, bias=P)
    return fill(hip.WinAttnDesc(), **merged(base, kw))


WIN = [
    dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(scale=None), dict(bias=None), dict(mode=2), dict(mode=-1), dict(hd=16),
    dict(B_=0), dict(nH=0), dict(N=0), dict(N=193), dict(mask=P, nW=0), dict(mask=P, nW=3), dict(mode=SEW, Tq=0, N1=64),
    dict(mode=SEW, Tq=2, N1=0), dict(mode=SEW, Tq=2, N1=63), dict(row_map=P), dict(mode=SEW, Tq=2, N1=64, row_map=P, pad_qkv=P),
    dict(q=ODD16), dict(mode=SEW, Tq=2, N1=64, q=ODD4), dict(out=ODD4),
    dict(q=None, mode=2), dict(mode=2, hd=16), dict(hd=16, row_map=P), dict(row_map=P, q=ODD16), dict(mask=P, nW=3, out=ODD4),
]


def call_desc(fn, make):
    return lambda lib, v: getattr(lib, fn)(C.byref(make(**copy.deepcopy(v))), None)


def call_args(fn, make):
    return lambda lib, v: getattr(lib, fn)(*make(**copy.deepcopy(v)))


ENTRIES = {
    "head_conv_sn": (call_desc("sdf_head_conv_sn_fwd", head_desc), HEAD),
    "pred_head": (call_desc("sdf_pred_head_fwd", pred_desc), PRED),
    "spike_gemm_16bit": (call_desc("sdf_spike_gemm_fwd", gemm_desc), GEMM),
    "spike_conv2d_16bit": (call_desc("sdf_spike_conv2d_fwd", conv_desc), CONV),
    "qk_gate": (call_args("sdf_qk_gate_fwd", lambda **kw: gate_args(False, **kw)), GATE),
    "qk_gate_strided": (call_args("sdf_qk_gate_strided_fwd", lambda **kw: gate_args(True, **kw)), GATE_STRIDED),
    "qk_attn": (call_desc("sdf_qk_attn_fwd", attn_desc), ATTN),
    "ms_mlp": (call_desc("sdf_ms_mlp_fwd", mlp_desc), MLP),
    "layer_norm": (call_args("sdf_layer_norm_fwd", ln_args), LN),
    "win_attn": (call_desc("sdf_win_attn_fwd", win_desc), WIN),
}
DESC_ENTRIES = {"head_conv_sn": "sdf_head_conv_sn_fwd", "pred_head": "sdf_pred_head_fwd", "spike_gemm_16bit": "sdf_spike_gemm_fwd",
                "spike_conv2d_16bit": "sdf_spike_conv2d_fwd", "qk_attn": "sdf_qk_attn_fwd", "ms_mlp": "sdf_ms_mlp_fwd",
                "win_attn": "sdf_win_attn_fwd"}
NEURON_ENTRIES = ("head_conv_sn", "pred_head", "spike_gemm_16bit", "spike_conv2d_16bit", "qk_gate", "qk_gate_strided", "qk_attn", "ms_mlp")


def refusal_codes(lib, key):
    call, vectors = ENTRIES[key]
    return [call(lib, v) for v in vectors]


@pytest.mark.parametrize("key", list(ENTRIES))
def test_refusals_before_any_launch(lib, golden, key):
    _, vectors = ENTRIES[key]
    if key in DESC_ENTRIES:
        assert getattr(lib, DESC_ENTRIES[key])(None, None) == E_NULL
    want = golden["refusals"][key]
    assert len(vectors) >= 15 and len(want) == len(vectors)
    got = refusal_codes(lib, key)
    for v, g, w in zip(vectors, got, want):
        assert g < 0, ("reached a launch", key, v, g)
        assert g == w, (key, v, g, w)
    assert {E_NULL, E_SHAPE, E_ALIGN} <= set(want)
    if key in NEURON_ENTRIES:
        assert E_DTYPE in want


if __name__ == "__main__":                              # record: run with SDF_HIP_LIB naming a build of the commit before the refactor
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sdformerflow_amd import hip
    assert not torch.cuda.is_available() and not [n for n in os.environ if n.startswith("SDF_") and n != "SDF_HIP_LIB"]
    codes = {key: refusal_codes(hip.lib(), key) for key in ENTRIES}
    assert all(c < 0 for v in codes.values() for c in v), {k: [(i, c) for i, c in enumerate(v) if c >= 0] for k, v in codes.items()}
    with open(GOLDEN, "w") as f:
        json.dump({"refusals": codes}, f, separators=(",", ":"))
        f.write("\n")
