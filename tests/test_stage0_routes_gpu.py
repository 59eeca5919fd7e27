"""Launches of the stage-0, head and tail kernels, pinned kernel by kernel: direct calls of hip.head_conv_sn, hip.pred_head, hip.qk_attn,
hip.ms_mlp and hip.layer_norm at the smallest shapes their rules admit, each asserting through hip.launch_log() the LITERAL list of
launches - workgroups, threads, dynamic LDS bytes, kernel with its template arguments - that the library made before the template
dispatch of these kernels was stated once (csrc/host_launch.h).  A call the library refuses stands in the list as "rc <code>" behind
whatever it launched first.  The lists stand in tests/golden/stage0_routes.json, one case per line, recorded on an MI355X with
SDF_HIP_LIB naming a build of the commit before the refactor: `PYTHONPATH=. python tests/test_stage0_routes_gpu.py [file]` writes them.

  * head convolution: B = 1, H = 2; T in {5, 10, 20} x the four (Cin, Cout) pairs x LIF with a soft reset (the `fast` form), LIF with a
    hard reset, IF and PSN (where PSN has no kernel the case records what the library does instead) - at W = 32 (the matrix-pipe
    kernels), at W = 16 and under SDF_HEAD_MFMA=0 (the other kernel);
  * prediction head: B = 1, h = 2, w = 4; D in {5, 10, 20} x Cin in {96, 192, 384} x the neuron classes 0 / 1 / 2; PSN at D = 20 is refused;
  * the one-launch first half of the QK attention: C = 96 (and 192 under SDF_QK_FRONT_ANY=1), T' = 2, one window, classes 0 / 1 / 2 with
    and without the tape; neurons of different classes take the three-launch form;
  * the one-launch MLP: C = 96 at T in {5, 10, 20} (192 under SDF_MLP_FUSED_ANY=1), classes 0 / 1 / 2, with and without the tape, one and
    three bf16 planes at T = 10; sn1 / sn2 of different classes take the three-launch form;
  * layer norm: 3 rows of C = 64 ... 512 in steps of 64 (1 ... 8 float4 per lane at 16 lanes per row) and C = 576, 1024, 2048 (64 lanes).

Every case runs twice into fresh buffers: the same launches and bit-equal outputs.  No numeric comparison: parity of the head
convolution, the prediction head, the one-launch QK front, the one-launch MLP and the token gate is test_stage0_parity_gpu.py's, every
instantiation listed here against the oracle (with test_hip_kernels.py::test_head_conv_bn_neuron, test_pred_head_gpu.py,
test_qk_front_gpu.py and test_ms_mlp_fused_gpu.py at the workload's shapes); the layer norm's is test_dense_linear_gpu.py's.  The
streaming GEMM and the window attention are pinned by test_spike_gemm_routes_gpu.py and test_win_attn_fwd_gpu.py."""
import json
import os

import pytest
import torch

from routes_common import DEV, logged, neuron, rnd
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage0_routes.json")
SWITCHES = ("SDF_HEAD_MFMA", "SDF_QK_FRONT", "SDF_QK_FRONT_ANY", "SDF_MLP_FUSED", "SDF_MLP_FUSED_ANY", "SDF_WIDE", "SDF_RES", "SDF_GEMM_CFG",
            "SDF_GEMM_WS", "SDF_GEMM_WGS")
PAIRS = ((2, 48), (2, 32), (2, 64), (4, 48))


class _L:
    """a linear layer as 16-bit planes + its BatchNorm (no int8 digits: the wide-stage kernels are not asked)"""

    def __init__(self, N, K, planes=2, bias=False):
        self.N, self.K = N, K
        self.Wp = hip.split_weight(rnd((N, K)), planes)
        self.alpha, self.beta = rnd((N,), 0.5, 1.5), rnd((N,), -0.2, 0.2)
        self.bias = rnd((N,)) if bias else None


# ------------------------------------------------------------------------------------------------------------------ the calls
def head(T, pair, name, W):
    Cin, Cout = pair
    x, w, n = rnd((T, 2, W, Cin), -0.5, 1.0), rnd((Cout, Cin, 3, 3), -0.5, 0.5), neuron(name, T)
    al, be = rnd((Cout,), 0.5, 1.5), rnd((Cout,), -0.2, 0.2)
    return lambda: (hip.head_conv_sn(x, w, 1, T, 2, W, n, al, be),)


def pred(D, Cin, name):
    z, wgt, bias, n = rnd((1, D, 2, 4, Cin), -0.5, 1.0), rnd((2, Cin)), rnd((2,)), neuron(name, D)
    return lambda: hip.pred_head(z, wgt, bias, n, 4, 8, want_pred=True, keep=True)


def attn(Cc, names, tape=False):
    nH, Tq, window = Cc // 32, 2, (2, 5, 5)
    N1 = window[1] * window[2]
    x = rnd((1, 2, 5, 5, Cc), -0.5, 1.0)
    plin, q_lin, k_lin, pe = _L(Cc, Cc, bias=True), _L(Cc, Cc), _L(Cc, Cc), rnd((Tq * N1, Cc))
    rowmap, B_ = hip.window_slice_map(1, 2, 5, 5, window, (0, 0, 0), DEV)
    ns = [neuron(n, Tq) for n in names]

    def call():
        keep = [] if tape else None
        y = hip.qk_attn(x.clone(), rowmap, B_, Tq, N1, nH, plin, *ns, q_lin=q_lin, k_lin=k_lin, pe=pe, keep_ws=keep)
        n, qk = Tq * B_ * N1 * Cc, (Tq * B_ * N1 * Cc + 255) // 256 * 256      # the tape: E, then q | k at the next 256-byte boundary
        return (y, *(t for ws in keep or () for t in (ws[:n], ws[qk:qk + 2 * n])))
    return call


def mlp(Cc, D, names, tape=False, planes=2):
    fc1, fc2 = _L(4 * Cc, Cc, planes), _L(Cc, 4 * Cc, planes)
    x, n1, n2 = rnd((1, D, 3, 5, Cc), -0.5, 1.0), neuron(names[0], D), neuron(names[1], D)

    def call():
        keep = [] if tape else None
        y = hip.ms_mlp(x.clone(), fc1, fc2, n1, n2, keep_ws=keep)
        n, s2 = D * 15 * Cc, (D * 15 * Cc + 255) // 256 * 256                  # the tape: SN1's spikes, then SN2's at the next 256-byte boundary
        return (y, *(t for ws in keep or () for t in (ws[:n], ws[s2:s2 + 4 * n])))
    return call


def ln(Cc):
    x, g, b = rnd((3, Cc), -1.0, 1.0), rnd((Cc,), 0.5, 1.5), rnd((Cc,))
    return lambda: (hip.layer_norm(x, g, b, 1e-5),)


# name: (switches, the call)
CASES = {}
for T in (5, 10, 20):
    for pair in PAIRS:
        for name in ("lif", "lif_hard", "if", "psn"):
            tag = f"T{T}_c{pair[0]}x{pair[1]}_{name}"
            CASES[f"head_mfma_{tag}"] = ({}, lambda T=T, pair=pair, name=name: head(T, pair, name, 32))
            CASES[f"head_w16_{tag}"] = ({}, lambda T=T, pair=pair, name=name: head(T, pair, name, 16))
            CASES[f"head_nomfma_{tag}"] = ({"SDF_HEAD_MFMA": "0"}, lambda T=T, pair=pair, name=name: head(T, pair, name, 32))
for D in (5, 10, 20):
    for Cin in (96, 192, 384):
        for name in ("lif", "psn", "lif_hard"):
            CASES[f"pred_D{D}_c{Cin}_{name}"] = ({}, lambda D=D, Cin=Cin, name=name: pred(D, Cin, name))
for name in ("lif", "psn", "lif_hard"):
    for tape in (False, True):
        CASES[f"qk_front_c96_{name}{'_tape' if tape else ''}"] = ({}, lambda name=name, tape=tape: attn(96, (name,) * 4, tape))
    CASES[f"qk_front_c192_{name}"] = ({"SDF_QK_FRONT_ANY": "1"}, lambda name=name: attn(192, (name,) * 4))
CASES["qk_front_mixed_classes"] = ({}, lambda: attn(96, ("lif", "lif_hard", "lif_hard", "lif")))
for name in ("lif", "psn", "lif_hard"):
    for D in (5, 10, 20):
        for tape in (False, True):
            CASES[f"mlp_c96_T{D}_{name}{'_tape' if tape else ''}"] = ({}, lambda D=D, name=name, tape=tape: mlp(96, D, (name,) * 2, tape))
    CASES[f"mlp_c192_{name}"] = ({"SDF_MLP_FUSED_ANY": "1"}, lambda name=name: mlp(192, 10, (name,) * 2))
    for planes in (1, 3):
        CASES[f"mlp_c96_planes{planes}_{name}"] = ({}, lambda name=name, planes=planes: mlp(96, 10, (name,) * 2, planes=planes))
CASES["mlp_mixed_classes"] = ({}, lambda: mlp(96, 10, ("lif", "if")))
for Cc in (64, 128, 192, 256, 320, 384, 448, 512, 576, 1024, 2048):
    CASES[f"layer_norm_c{Cc}"] = ({}, lambda Cc=Cc: ln(Cc))


def launches(name, monkeypatch):
    """the case run twice: the launches (the same both times) and whether the outputs were bit-equal"""
    env, make = CASES[name]
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(0)
    call = make()
    torch.cuda.synchronize()
    first, out1 = logged(call)
    second, out2 = logged(call)
    assert first == second, (name, first, second)
    outs = [(a, b) for a, b in zip(out1, out2) if a is not None]
    assert len(out1) == len(out2) and all(a.data_ptr() != b.data_ptr() and torch.equal(a, b) for a, b in outs), (name, "outputs differ between two runs")
    return first


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_launches_are_those_recorded(name, monkeypatch, golden):
    got = launches(name, monkeypatch)
    print(name, got)
    assert got == golden[name]


def test_the_cases_reach_every_route(golden):
    """The table itself: what the cases are asked to reach, read off the recorded kernel names."""
    assert set(golden) == set(CASES)
    seen = {line.split(" ", 3)[3] for want in golden.values() for line in want if not line.startswith("rc ")}
    args = lambda kernel: {tuple(a.strip() for a in s[len(kernel) + 1:-1].split(",")) for s in seen if s.startswith(kernel + "<")}
    pairs = {(str(ci), str(co)) for ci, co in PAIRS}
    assert {a[:3] for a in args("head_conv_mfma_kernel")} == {(t, ci, co) for t in ("5", "10", "20") for ci, co in pairs}
    assert {a[3] for a in args("head_conv_mfma_kernel")} == {"true", "false"}
    assert args("head_conv_mfma_psn_kernel") == {(t, "2", co) for t in ("5", "10") for co in ("48", "32")}
    assert args("head_conv_sn_kernel") == {(t, str(int(co) // 16), ci) for t in ("5", "10", "20") for ci, co in pairs}
    assert args("pred_head_kernel") == {(d, l, n) for d in ("5", "10", "20") for l in ("8", "16", "32") for n in ("0", "1", "2")} - \
        {("20", l, "1") for l in ("8", "16", "32")}
    for D in (5, 10):
        assert not any(line.startswith("rc ") for line in golden[f"pred_D{D}_c96_psn"])
    for Cin in (96, 192, 384):
        assert golden[f"pred_D20_c{Cin}_psn"] == [f"rc {hip.E_SHAPE}"]
    assert args("qk_front_kernel") == {(n, k) for n in ("0", "1", "2") for k in ("true", "false")}
    assert len(golden["qk_front_mixed_classes"]) == 5 and not any("qk_front" in line for line in golden["qk_front_mixed_classes"])
    m = args("ms_mlp_fused_kernel")
    assert {(a[0], a[1]) for a in m} == {("2", "5"), ("2", "10"), ("2", "20"), ("1", "10"), ("3", "10")} and {a[2] for a in m} == {"6", "12"}
    assert {a[7] for a in m} == {"0", "1", "2"} and {a[8] for a in m} == {"true", "false"} and not any(a[1] == "20" and a[7] == "1" for a in m)
    assert len(golden["mlp_mixed_classes"]) == 3 and not any("ms_mlp_fused" in line for line in golden["mlp_mixed_classes"])
    assert args("layer_norm_kernel") == {("16", v) for v in ("1", "2", "3", "4", "6", "8")} | {("64", v) for v in ("3", "4", "8")}


if __name__ == "__main__":                              # record: run with SDF_HIP_LIB naming a build of the commit before the refactor
    import sys

    class _Env:
        """monkeypatch's two calls for a plain run"""

        def setenv(self, k, v):
            os.environ[k] = v
            hip.reload_switches()

        def delenv(self, k, raising=True):
            if os.environ.pop(k, None) is not None:
                hip.reload_switches()

    rec = {name: launches(name, _Env()) for name in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items()) + "\n}\n")
