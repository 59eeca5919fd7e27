"""The launch schedule of sdformerflow_amd/engine.py, checked without a GPU.

(1) The engine's call trace on meta tensors (tests/golden/make_engine_call_trace.py: which entry point, weight representation and
    image count every 3x3 convolution, decoder level and prediction head gets, over 21 cases: batch, replicas, PSN, T = 5 / 20, no
    digit planes, the concatenation path, the SDF_* route switches) equals tests/golden/engine_call_trace.json record for record.
(2) The replica rule holds on the route functions themselves, for every layer the trace went through.
(3) The routing policy is stated in the route functions only."""
import ast
import importlib.util
import inspect
import json
import os
import re

import pytest

from sdformerflow_amd import engine as E, hip

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
spec = importlib.util.spec_from_file_location("make_engine_call_trace", os.path.join(GOLDEN, "make_engine_call_trace.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


@pytest.fixture(scope="module")
def traced():
    """(trace of every case, the route questions asked on the way: {(switches, function name, arguments)})."""
    asked, switches = set(), [()]
    real = {n: getattr(E, n) for n in ("conv3x3_route", "deconv_route")}

    def spy(name):
        def f(*a, **k):
            args = inspect.signature(real[name]).bind(*a, **k)
            args.apply_defaults()
            asked.add((switches[0], name, tuple(args.arguments.values())))
            return real[name](*a, **k)
        return f
    try:
        for n in real:
            setattr(E, n, spy(n))
        engines, trace = {}, {}
        for c in T.cases():
            switches[0] = tuple(sorted(c[-1].items()))
            trace[c[0]] = T.trace_case(*c[1:], engines=engines)
    finally:
        for n, f in real.items():
            setattr(E, n, f)
    return trace, asked


def test_call_trace_is_the_recorded_one(traced):
    want = json.load(open(os.path.join(GOLDEN, "engine_call_trace.json")))
    got = json.loads(T.dumps(traced[0]))                                 # (through JSON: tuples and lists compare alike)
    assert list(got) == list(want)
    for case in want:
        for part in want[case]:
            g, w = got[case][part], want[case][part]                      # (lines, or "= <the earlier case with the same lines>")
            assert type(g) is type(w) and len(g) == len(w), (case, part, g if isinstance(g, str) else len(g), w if isinstance(w, str) else len(w))
            for i, (gl, wl) in enumerate([(g, w)] if isinstance(w, str) else zip(g, w)):
                assert gl == wl, (case, part, i, gl, wl)


def _convs(trace, case, part, **match):
    return [r for r in trace[case][part] if r["fn"] == "spike_conv2d" and all(r[k] == v for k, v in match.items())]


def test_trace_records_what_it_should(traced):
    """Known launches of the shipped model, stated by hand: the harness records them as they are."""
    t = traced[0]
    c96 = dict(Cin=96, N=96, stride=1, H=144, W=192)
    assert [(r["w"], r["imgs"], r["sn"]) for r in _convs(t, "c1_lif", "patch_embed", **c96)] == [("digits_rm", 10, "lif")] * 4
    assert [(r["imgs"], r["x_img0"]) for r in _convs(t, "c1_lif_R40", "patch_embed", **c96)] == [(200, 0), (200, 200)] * 4
    psn = t["c1_psn"]["patch_embed"]
    i = psn.index(_convs(t, "c1_psn", "patch_embed", **c96)[0])
    assert (psn[i]["w"], psn[i]["epi"], psn[i]["bn"]) == ("digits_rm", "fp32", True) and (psn[i + 1]["fn"], psn[i + 1]["bn"]) == ("neuron_fwd", False)
    assert [(r["imgs"], r["epi"]) for r in _convs(t, "c4_lif_B4", "patch_embed", Cin=96, stride=1, resid=True)] == [(40, "both")] * 4
    assert [(r["w"], r["imgs"]) for r in _convs(t, "c1_lif_R10", "unet_tail", Cin=768)] == [("digits_tiled", 100)] * 4
    assert [r["imgs"] for r in _convs(t, "c1_lif_R40", "unet_tail", Cin=768)] == [200] * 8
    assert [(r["w"], r["imgs"], r["epi"]) for r in _convs(t, "c1_lif_R10", "patch_embed", Cin=96, stride=2)] == [("digits_rm", 100, "fp32")]
    small = dict(Cin=96, N=96, stride=1, H=72, W=96)
    assert [(r["w"], r["imgs"], r["sn"]) for r in _convs(t, "small_lif_R3", "patch_embed", **small)] == [("planes16x2", 30, "lif")] * 4
    assert [r["imgs"] for r in _convs(t, "small_lif_R4", "patch_embed", **small)] == [20] * 8
    assert [r["imgs"] for r in _convs(t, "planes3_lif_R3", "patch_embed", **c96)] == [10] * 12
    for case, k in (("c1_lif", 1), ("c1_lif_R10", 10)):
        tail = [(r["fn"], r.get("w"), r.get("M", r.get("imgs")), r.get("epi")) for r in t[case]["unet_tail"]]
        assert tail == [("neuron_fwd", None, None, None)] + \
            [("spike_conv2d", "digits_tiled", 10 * k, e) for e in ("spikes", "both", "spikes", "fp32")] + [("neuron_multi_fwd", None, None, None)] + \
            [("spike_gemm", "digits_tiled", 1080 * k, None), ("deconv_col2im", None, 10 * k, None), ("pred_head", None, None, None),
             ("spike_gemm", "digits_rm", 4320 * k, None), ("deconv_col2im", None, 10 * k, None), ("pred_head", None, None, None),
             ("spike_gemm", "digits_rm", 17280 * k, None), ("deconv_col2im", None, 10 * k, None), ("pred_head", None, None, None),
             ("spike_deconv3x3s2", "digits_rm", 10 * k, None), ("pred_head", None, None, None)], case
        assert len(t[case]["unet_tail"][5]["descriptors"]) == 5
    # 75 x 100 features: levels 1 and 3 concatenate (one neuron launch on the concatenation), level 0 writes y and skip itself,
    # level 2 gets [y | prediction] from the head above and writes its skip slice
    assert [(r["fn"], r.get("nb")) for r in t["odd_lif"]["unet_tail"][5:] if r["fn"] in ("neuron_fwd", "neuron_multi_fwd")] == \
        [("neuron_fwd", 130), ("neuron_fwd", 130), ("neuron_fwd", 1), ("neuron_fwd", 1900), ("neuron_fwd", 1)]
    assert [r["feeds_next"] for r in t["odd_lif"]["unet_tail"] if r["fn"] == "pred_head"] == [False, True, False, False]


def test_replicas_route_every_layer_like_one_sample(traced):
    """For every layer the trace went through and every replica count: the kernel form is the batch-1 form, the samples per launch
    divide the batch, and such a chunk on its own is routed the same way, as one launch."""
    layers = {(sw, name, args[1:-1]) for sw, name, args in traced[1]}      # (without the batch size and the replicas flag)
    assert sum(name == "conv3x3_route" for _, name, _ in layers) >= 20 and sum(name == "deconv_route" for _, name, _ in layers) >= 8
    for sw, name, args in sorted(layers, key=repr):
        route = getattr(E, name)
        with hip.scoped_switches(**dict(sw)):
            one = route(1, *args, replicas=True)
            assert one == route(1, *args, replicas=False)
            D = args[0]
            for R in (2, 3, 4, 7, 10, 40):
                r = route(R, *args, replicas=True)
                n = r.samples if name == "conv3x3_route" else r.images // D
                assert r.form == one.form and n >= 1 and R % n == 0, (name, args, R, r, one)
                assert route(n, *args, replicas=True) == r, (name, args, R, n)
                if name == "deconv_route":
                    assert r.cp == one.cp and r.images % D == 0


def _calls_by_function(tree):
    """{called name: {names of the top-level functions / methods whose body calls it}} of a module."""
    out = {}
    for top in ast.walk(tree):
        if isinstance(top, ast.FunctionDef):
            for node in ast.walk(top):
                if isinstance(node, ast.Call):
                    f = node.func
                    name = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)
                    out.setdefault(name, set()).add(top.name)
    return out


def test_policy_is_stated_in_the_route_functions_only():
    src = inspect.getsource(E)
    calls = _calls_by_function(ast.parse(src))
    conv, deconv = {"conv3x3_route", "asked"}, {"deconv_route"}            # (`asked`: the route function's own inner function)
    for pred, where in (("conv_wres_applicable", conv), ("smallm_conv_applicable", conv), ("smallm_gemm_applicable", deconv),
                        ("smallm_gemm_rows_ok", deconv), ("res_gemm_applicable", deconv), ("deconv2x2_applicable", deconv)):
        assert calls[pred] <= where, (pred, calls[pred])
    assert calls["_largest_divisor"] <= conv | deconv
    for gone in ("_conv3x3_chunks", "_digit_chunk", "_fusable", "_decoder_geometry", "_dst", "_rb"):
        assert not re.search(rf"\b{gone}\b", src), gone
    assert "_conv3x3" not in calls["_conv3x3"]                             # (it does not call itself)
    longest = max((n.end_lineno - n.lineno + 1, n.name) for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef))
    assert longest[0] < 158, longest                                       # (the one-function unet_tail this schedule had)
