"""Cases, inputs and references of tests/test_neuron_parity_gpu.py: value parity of every instantiation of the stand-alone neuron
kernels of the training path - csrc/neuron_bwd.hip (lif_bwd_kernel<T, PLIF>, psn_bwd_kernel<T, REDUCE, VEC>, psn_bwd_finish_kernel),
csrc/glif.hip (glif_fwd_kernel<T, U8>, glif_bwd_kernel<T>, glif_bwd_finish_kernel), csrc/qk_gate_train.hip
(qk_gate_train_kernel<TQ, BWD, PLIF>, gate_finish_kernel) and the PLIF training forward of csrc/neuron.hip (plif_fwd_kernel<T>).
Plain CPU code; the unmarked tests of tests/test_neuron_parity_gpu.py hold its premises without a GPU.

ENUMERATION.  The T lists are read from the text of csrc/host_launch.h (`SdfList<...> SDF_T_STREAM / SDF_T_GLIF / SDF_T_GATE`), the
neurons per lane of the reducing PSN backward from the text of `psn_reduce_vec` in csrc/neuron_bwd.hip; the grids are
`sdf_quad_blocks`, `psn_blocks` and `gate_blocks` as the dispatch code states them.  Every case carries `launches`, the
(kernel name with its template arguments, workgroups) rows hip.launch_log() must show; `instantiations()` is the set the dispatch code
can produce, and the CPU test holds the union of all cases' launches equal to it.

INPUTS.  Seeded synthetic.synth_uniform, four column blocks of every x overwritten (BLK columns each, `blocks(N)`):
  tie     x_0 = TIE_X with the threshold of the case set to the fp32 h_0 that x gives (`tie_threshold`), so h_0 - v_th == 0 exactly and
          `>= 0` must fire (GLIF: the threshold is a table entry, the x is searched as the fixtures' generator does);
  hard    a spike at every step, so the reset path carries gradient at every t;
  silent  never a spike;
  late    the first spike at the last step.
The gate's x are head sums of q, integers 0 .. 32: the blocks are (row, head) pairs whose 32 channels hold 1 / 32 / 0 / (0 .. 0, 32) ones and q
fires at 3 %, so a head sum is 0 in about four of ten pairs.  With the threshold at the h_0 of one spike the first step decides as the
shipped v_th = 0.1 does (any spike in the head opens the gate), and the membrane near the threshold is of order 1: its fp32 rounding,
2^-24 |h| per step, stays an order below the 1e-6 the surrogate's slope (at most 2 per unit of u) lets through to dL/dq.  (At a
threshold of 5.8, head sum 10, that rounding alone put dL/dq 1.0e-6 from the fp64 reference.)
dL/ds is uniform in [-1, 1]; `wide` cases draw sign * 10^U(-3, 3), six decades.

REFERENCE.  `reference` runs the per-step loop of the published equations under torch.autograd in fp64 (LIF / IF / ParametricLIF of
oracle/stubs/README.md, SLTT with v.detach() in the charge, GatedLIFNode as Spiking_submodules.py:152-180, PSN addmm, the gate
expression q.sum -> neuron -> repeat_interleave -> k.mul) with an ATan autograd.Function whose forward returns the FORCED decision of
the fp32 trajectory (neuron_bwd_ref.lif_forward_h, sdformer_oracle.glif_multistep, `plif_forward`, the charge_differences loop of
test_plif_train_gpu.py): nothing chaotic stands between the two sides.  It shares no line with neuron_bwd_ref.lif_backward, the
reverse recurrence written like neuron_step.h.  Parameters enter as one leaf PER TERM (k as (T, N), the GLIF table as (T, 5 + T, N), W as
(T, T, N)), so the gradient of a parameter is the sum of its leaf's gradient and the bound's scale, sum |terms|, the sum of its
absolute values.  The same loop in fp32 (`dtype=torch.float32`) measures the reference's own rounding for the T = 16, 20 bound."""
import functools
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

from oracle import neuron_bwd_ref as BW
from oracle import sdformer_oracle as O
from sdformerflow_amd.synthetic import synth_state_dict, synth_uniform as rnd

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sdformerflow_amd", "csrc")
GOLD = os.path.join(HERE, "golden")
ALPHA = 2.0
N_SMALL = 1028                                       # two workgroups, the second ragged (test_neuron_dispatch_gpu.py)
N_FINISH2 = 4 * 256 * 257                            # 257 partials: the finish kernels' strided loop takes a second turn
ROWS, CS = 9, (32, 96, 192, 384, 768)                # default gate
ROWS_FINISH2 = 8200                                  # C = 32: 8200 pairs * 8 lanes = 257 workgroups of partials
BLK, TIE_X, GATE_TIE = 16, 0.2, 1
RESETS = {"soft": None, "hard": 0.0, "hard005": 0.05}
PLIF_KS = {"k05": 0.0, "k03": 0.3, "k035": 0.35}     # w: k = sigmoid(0) = 0.5 and sigmoid(0.3) in the sweep; 0.35 is the PLIF fixture's
GATES = ("alpha", "beta", "gamma", "tau", "v_threshold", "linear_decay", "v_subreset", "conduct")


# ------------------------------------------------------------------ the dispatch code, read from its text
def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(None)
def t_lists():
    """{'STREAM': (1, 2, ...), 'GLIF': ..., 'GATE': ...} from the SdfList definitions of host_launch.h."""
    found = dict((m.group(2), tuple(int(v) for v in m.group(1).split(",")))
                 for m in re.finditer(r"SdfList<([\d,\s]+)>\s+SDF_T_(\w+)\s*\{", _text("host_launch.h")))
    assert set(found) == {"STREAM", "GLIF", "GATE"}, found
    return found


def _ternary(expr, T):
    """`T < m ? a : T <= n ? b : d` of a C constexpr over T."""
    if "?" not in expr:
        return int(expr)
    cond, rest = expr.split("?", 1)
    a, b = rest.split(":", 1)
    op, bound = re.fullmatch(r"\s*T\s*(<=|<)\s*(\d+)\s*", cond).groups()
    return int(a) if (T <= int(bound) if op == "<=" else T < int(bound)) else _ternary(b, T)


def psn_reduce_vec(T):
    m = re.search(r"constexpr int psn_reduce_vec\(int T\) \{ return ([^;]+); \}", _text("neuron_bwd.hip"))
    return _ternary(m.group(1), T)


def psn_vec(T, reduce):
    return psn_reduce_vec(T) if reduce and psn_reduce_vec(T) else 4


def quad_blocks(n):
    return (n // 4 + 255) // 256


def psn_blocks(T, N, reduce):
    return min((N // psn_vec(T, reduce) + 255) // 256, 512)


def gate_blocks(rows, Cc):
    return (rows * (Cc // 32) * 8 + 255) // 256


def tf(b):
    return "true" if b else "false"


def instantiations():
    """Every kernel<...> the dispatch code of the three files and sdf_plif_fwd can launch, as launch-log name parts."""
    L, out = t_lists(), set()
    for T in L["STREAM"]:
        out |= {f"lif_bwd_kernel<{T}, false>(", f"lif_bwd_kernel<{T}, true>(", f"plif_fwd_kernel<{T}>(", f"psn_bwd_kernel<{T}, false, 4>("}
        if psn_reduce_vec(T):
            out.add(f"psn_bwd_kernel<{T}, true, {psn_reduce_vec(T)}>(")
    for T in L["GLIF"]:
        out |= {f"glif_fwd_kernel<{T}, false>(", f"glif_fwd_kernel<{T}, true>(", f"glif_bwd_kernel<{T}>("}
    for T in L["GATE"]:
        out |= {f"qk_gate_train_kernel<{T}, {tf(b)}, {tf(p)}>(" for b in (False, True) for p in (False, True)}
    return out | {"psn_bwd_finish_kernel(", "glif_bwd_finish_kernel(", "gate_finish_kernel("}


# ------------------------------------------------------------------ cases
# family: lif | if | sltt | plif | psn | glif (stream kernels), gate_lif | gate_if | gate_plif | gate_psn; launches: the backward's rows,
# fwd_launches: the forward's (PSN: the reducing backward's, `launches` being the two non-reducing forms')
Case = namedtuple("Case", "family T N rows C reset detach tau kw wide seed launches fwd_launches")


def _case(family, T, N=N_SMALL, rows=0, C=0, reset="soft", detach=True, tau=2.0, kw=None, wide=False):
    seed = 7000 + 97 * T + 13 * list(RESETS).index(reset) + (5 if detach else 0) + int(tau) + (C or N) % 89 + (1 if wide else 0)
    fwd = []
    if family in ("lif", "if", "sltt"):
        la = [(f"lif_bwd_kernel<{T}, false>(", quad_blocks(N))]
    elif family == "plif":
        la = [(f"lif_bwd_kernel<{T}, true>(", quad_blocks(N)), ("psn_bwd_finish_kernel(", 1)]
        fwd = [(f"plif_fwd_kernel<{T}>(", quad_blocks(N))]
    elif family == "psn":                              # reducing launch (T <= 10), then the two non-reducing forms
        la = [(f"psn_bwd_kernel<{T}, false, 4>(", psn_blocks(T, N, False))]
        if psn_reduce_vec(T):
            fwd = [(f"psn_bwd_kernel<{T}, true, {psn_reduce_vec(T)}>(", psn_blocks(T, N, True)), ("psn_bwd_finish_kernel(", T * T + T)]
    elif family == "glif":
        la = [(f"glif_bwd_kernel<{T}>(", quad_blocks(N)), ("glif_bwd_finish_kernel(", 5 + T)]
        fwd = [(f"glif_fwd_kernel<{T}, {tf(u8)}>(", quad_blocks(N)) for u8 in (False, True)]
    else:
        plif, psn = family == "gate_plif", family == "gate_psn"
        la = [(f"qk_gate_train_kernel<{T}, true, {tf(plif)}>(", gate_blocks(rows, C))]
        la += [("gate_finish_kernel(", T * T + T)] if psn else [("gate_finish_kernel(", 1)] if plif else []
        fwd = [(f"qk_gate_train_kernel<{T}, false, {tf(plif)}>(", gate_blocks(rows, C))]
    return Case(family, T, N, rows, C, reset, detach, tau, tuple(sorted(dict(kw or {}).items())), wide, seed, tuple(la), tuple(fwd))


def name(c):
    parts = [c.family, f"T{c.T}", f"C{c.C}x{c.rows}" if c.C else f"N{c.N}"]
    if c.family not in ("psn", "glif", "gate_psn"):
        parts += [c.reset, "detach" if c.detach else "nodetach", f"tau{c.tau:g}"]
    return "-".join(parts + [f"{k}{v}" for k, v in c.kw] + (["wide"] if c.wide else []))


def settings(family):
    """(reset, detach, tau, kw) of one (family, T): the whole sweep the family has."""
    lif = family in ("lif", "gate_lif")
    for reset in RESETS:
        for detach in (True,) if family == "sltt" else (True, False):          # sdf_sltt_bwd has no detach argument
            if family in ("plif", "gate_plif"):
                for kn in ("k05", "k03"):
                    yield reset, detach, 2.0, {"k": kn}
            else:
                for tau in (2.0, 3.0) if lif or family == "sltt" else (2.0,):
                    yield reset, detach, tau, {}


@functools.lru_cache(None)
def stream_cases(family, T):
    """Small cases of one stream family at one T: the sweep, one six-decade case, and the large case at the smallest T of the list."""
    first = T == min(t_lists()["GLIF" if family == "glif" else "STREAM"])
    if family == "psn":
        out = [_case("psn", T), _case("psn", T, wide=True)]
        if T == 2:                                                            # VEC = 4: a second, ragged turn of the grid-stride loop
            out.append(_case("psn", T, N=4 * 512 * 256 + 1028))
        if T == min(t for t in t_lists()["STREAM"] if psn_reduce_vec(t) == 2):  # the first VEC = 2 instantiation, the same
            out.append(_case("psn", T, N=2 * 512 * 256 + 1028))
        return out
    if family == "glif":
        return [_case("glif", T), _case("glif", T, wide=True)] + ([_case("glif", T, N=N_FINISH2)] if first else [])
    out = [_case(family, T, reset=r, detach=d, tau=tau, kw=kw) for r, d, tau, kw in settings(family)]
    out.append(_case(family, T, reset="hard005", detach=False, kw=out[0].kw, wide=True))
    if family == "plif" and first:
        out.append(_case("plif", T, N=N_FINISH2, reset="hard005", detach=False, kw={"k": "k03"}))
    return out


@functools.lru_cache(None)
def gate_cases(family, Tq):
    out = []
    for Cc in CS:
        if family == "gate_psn":
            out.append(_case(family, Tq, rows=ROWS, C=Cc, kw={"W": "exact"}))
        else:
            out += [_case(family, Tq, rows=ROWS, C=Cc, reset=r, detach=d, tau=tau, kw=kw) for r, d, tau, kw in settings(family)]
    if family == "gate_psn":
        out.append(_case(family, Tq, rows=167, C=96, kw={"W": "random"}))        # the 16-ulp rule; rows as test_plif_train_gpu.py
        out.append(_case(family, Tq, rows=ROWS, C=96, kw={"W": "exact"}, wide=True))
    else:
        out.append(_case(family, Tq, rows=ROWS, C=96, reset="hard005", detach=False, kw=out[0].kw, wide=True))
    if family in ("gate_psn", "gate_plif") and Tq == min(t_lists()["GATE"]):
        kw = {"W": "exact"} if family == "gate_psn" else {"k": "k03"}
        out.append(_case(family, Tq, rows=ROWS_FINISH2, C=32, reset="hard005", detach=False, kw=kw))
    return out


STREAM_FAMILIES = ("lif", "if", "sltt", "plif", "psn")
GATE_FAMILIES = ("gate_lif", "gate_if", "gate_plif", "gate_psn")


def groups():
    """[(family, T)] - one GPU test each."""
    L = t_lists()
    return ([(f, T) for f in STREAM_FAMILIES for T in L["STREAM"]] + [("glif", T) for T in L["GLIF"]] +
            [(f, T) for f in GATE_FAMILIES for T in L["GATE"]])


def cases_of(family, T):
    return gate_cases(family, T) if family.startswith("gate_") else stream_cases(family, T)


def all_cases():
    return [c for f, T in groups() for c in cases_of(f, T)]


# ------------------------------------------------------------------ fp32 trajectories (the kernels' documented operation order)
def plif_forward(x, k, v_th, v_reset):
    """(d_t, h_t, s_t) of the PLIF forward in fp32: the charge_differences loop of test_plif_train_gpu.py, keeping h and s too."""
    v = torch.full_like(x[0], 0.0 if v_reset is None else v_reset)
    ds, hs, ss = [], [], []
    for t in range(x.shape[0]):
        d = x[t] - v if v_reset in (None, 0.0) else x[t] - (v - v_reset)
        h = v + d * k
        s = (h - v_th >= 0).float()
        v = h - s * v_th if v_reset is None else (1.0 - s) * h + s * v_reset
        ds.append(d), hs.append(h), ss.append(s)
    return torch.stack(ds), torch.stack(hs), torch.stack(ss)


def plif_k(c):
    """k = sigmoid(w) as the fp32 value the module computes."""
    return torch.sigmoid(torch.tensor(PLIF_KS[dict(c.kw)["k"]], dtype=torch.float32))


def kind_of(c):
    return {"lif": "lif", "sltt": "lif", "if": "if", "plif": "plif", "gate_lif": "lif", "gate_if": "if", "gate_plif": "plif"}[c.family]


def trajectory(c, x, v_th):
    """(h, s) in fp32 of the LIF / IF / PLIF neuron of the case on x (T, ...)."""
    vr = RESETS[c.reset]
    if kind_of(c) == "plif":
        return plif_forward(x, plif_k(c), v_th, vr)[1:]
    return BW.lif_forward_h(x, c.tau, v_th, vr, kind_of(c))


def tie_threshold(c, x_tie):
    """The threshold of the case: the fp32 h_0 of a neuron whose first input is x_tie, so that h_0 - v_th == 0 there."""
    h, _ = trajectory(c, torch.tensor([[x_tie]], dtype=torch.float32), 1e9)
    return float(h[0, 0])


def blocks(n):
    """Column ranges of the four overwritten blocks among n columns."""
    return {k: slice(i * BLK, (i + 1) * BLK) for i, k in enumerate(("tie", "hard", "silent", "late"))} if n >= 4 * BLK else {}


def grad_like(shape, seed, wide):
    if not wide:
        return rnd(shape, seed, -1.0, 1.0)
    return torch.sign(rnd(shape, seed, -1.0, 1.0)) * torch.pow(10.0, rnd(shape, seed + 1, -3.0, 3.0))


@functools.lru_cache(None)
def glif_table(T):
    """(table [L, Dk, g, R, th, c_0 ..], logits as a state dict, tie x): the fixture's logits at the T it holds, else the first
    seeded synth_state_dict draw for which an fp32 x with (0 - Dk) + x * c_0 - th == 0 exists (the generator's search)."""
    GG = np.load(os.path.join(GOLD, "glif_grads.npz"))
    if f"T{T}_tab" in GG.files:
        sd = {"spiking_neuron." + k: torch.from_numpy(GG[f"T{T}/spiking_neuron.{k}"]) for k in GATES}
        tab = table_of(sd)
        assert torch.equal(tab, torch.from_numpy(GG[f"T{T}_tab"]))
        return tab, sd, float(GG[f"T{T}_tie_x"])
    for salt in range(16):
        drawn = synth_state_dict({"glif_node." + k: (T,) if k == "conduct" else () for k in GATES}, salt=100 * T + salt)
        sd = {"spiking_neuron." + k: 40.0 * drawn["glif_node." + k].float() for k in GATES}     # N(0, 0.02) draws -> logits of N(0, 0.8)
        tab = table_of(sd)
        Dk, th, c0 = tab[1], tab[4], tab[5]
        xs = np.float32((float(th) + float(Dk)) / float(c0))
        cand = [xs]
        for direction in (np.float32(np.inf), np.float32(-np.inf)):
            v = xs
            for _ in range(64):
                v = np.nextafter(v, direction)
                cand.append(v)
        xv = torch.from_numpy(np.array(cand, dtype=np.float32))
        hit = ((torch.zeros(()) - Dk) + xv * c0) - th == 0
        if bool(hit.any()):
            return tab, sd, float(xv[hit][0])
    raise AssertionError("no seeded GLIF table with an exact fp32 tie")


def table_of(sd):
    """The derived table from the gate logits, the products in the reference's order (Spiking_submodules.py:153-162)."""
    s = {k: torch.sigmoid(sd["spiking_neuron." + k].float()) for k in GATES}
    head = torch.stack([1 - s["alpha"] * (1 - s["tau"]), (1 - s["alpha"]) * s["linear_decay"], s["gamma"],
                        (1 - s["gamma"]) * s["v_subreset"], s["v_threshold"]])
    return torch.cat([head, 1 - s["beta"] * (1 - s["conduct"])])


def psn_wb(T, seed, exact, centre=None):
    """(W (T, T), b (T)).  centre: a positive diagonal and b = -centre * (row sums of W) + a draw, so that h = b + W s changes sign
    around inputs of that size.  exact: multiples of 2^-6 with |W| < 1, so W times integer head sums is exact in fp32 in any order."""
    W, b = rnd((T, T), seed, -0.9, 0.9), rnd((T,), seed + 1, -3.0, 1.0)
    if centre is not None:
        W[range(T), range(T)] = W.diagonal().abs().clamp_min(0.25)
        b = 0.1 * b - centre * W.sum(1)
    if exact:
        W, b = torch.round(W * 64) / 64, torch.round(b * 64) / 64
    return W, b


Inputs = namedtuple("Inputs", "x g v_th aux")       # stream: x (T, N); gate: x = q, aux = {'k': k spikes, ...}


@functools.lru_cache(None)
def inputs(c):
    if c.family.startswith("gate_"):
        return _gate_inputs(c)
    T, N = c.T, c.N
    x, g, b = rnd((T, N), c.seed, -0.3, 0.6), grad_like((T, N), c.seed + 1000, c.wide), blocks(N)
    if c.family == "glif":
        tab, sd, tie_x = glif_table(T)
        x = 3.0 * x
        x[0, b["tie"]], x[:, b["hard"]], x[:, b["silent"]], x[:, b["late"]] = tie_x, 2.5, -0.5, 0.0
        x[T - 1, b["late"]] = 8.0
        return Inputs(x, g, float(tab[4]), {"tab": tab, "sd": sd})
    if c.family == "psn":
        W, bb = psn_wb(T, c.seed + 50, False)
        W, bb = 0.5 * W, 0.2 * bb
        x[0, b["tie"]], x[:, b["hard"]], x[:, b["silent"]], x[:, b["late"]] = TIE_X, 2.5, -0.2, 0.0
        x[T - 1, b["late"]] = 2.5
        return Inputs(x, g, 0.0, {"W": W, "b": bb})
    v_th = tie_threshold(c, TIE_X)
    x[0, b["tie"]], x[:, b["hard"]], x[:, b["silent"]], x[:, b["late"]] = TIE_X, 2.5, -0.2, 0.0
    x[T - 1, b["late"]] = 2.5
    return Inputs(x, g, v_th, {})


def _gate_inputs(c):
    """q, k spikes (Tq, rows, C) and dL/de; the first four (row, head) pairs' head sums are 1 (the tie), 32, 0 and (0 .., 32)."""
    Tq, rows, Cc = c.T, c.rows, c.C
    q = (rnd((Tq, rows, Cc), c.seed, 0.0, 1.0) < 0.03).float()
    k = (rnd((Tq, rows, Cc), c.seed + 1, 0.0, 1.0) < 0.4).float()
    pairs = q.view(Tq, rows * (Cc // 32), 32)
    pairs[:, 0] = 0.0
    pairs[:, 0, :GATE_TIE] = 1.0
    pairs[:, 1], pairs[:, 2], pairs[:, 3] = 1.0, 0.0, 0.0
    pairs[Tq - 1, 3] = 1.0
    g = grad_like((Tq, rows, Cc), c.seed + 1000, c.wide)
    if c.family == "gate_psn":
        W, b = psn_wb(Tq, c.seed + 50, dict(c.kw)["W"] == "exact", centre=1.0)
        return Inputs(q, g, 0.0, {"k": k, "W": W, "b": b})
    return Inputs(q, g, tie_threshold(c, float(GATE_TIE)), {"k": k})


def head_sums(q):
    Tq, rows, Cc = q.shape
    return q.reshape(Tq, rows, Cc // 32, 32).sum(-1)


def psn_gate_h32(sums, W, b):
    """h = b + W s as the kernel's fma chain (k ascending) in fp32: the product of a 24-bit by a 6-bit number and its sum with an fp32
    are exact in fp64, so rounding that sum once is the fused multiply-add.  Exact in any order for the `exact` weights."""
    h = []
    for t in range(sums.shape[0]):
        hh = b[t].expand_as(sums[0]).clone()
        for k in range(sums.shape[0]):
            hh = (hh.double() + W[t, k].double() * sums[k].double()).float()
        h.append(hh)
    return torch.stack(h)


def decisions(c):
    """The fp32 trajectory's spike decisions of the case (what the reference is forced to), and for the random-W PSN gate the mask
    of decisions kept under the 16-ulp rule (|h| beyond 16 * 2^-23 * max(rms h, 0.1)); None where no decision enters the result."""
    i = inputs(c)
    if c.family == "psn":
        return None, None
    if c.family == "glif":
        return O.glif_multistep(i.x, i.aux["sd"], "spiking_neuron."), None
    x = head_sums(i.x) if c.family.startswith("gate_") else i.x
    if c.family == "gate_psn":
        h = psn_gate_h32(x, i.aux["W"], i.aux["b"])
        keep = h.abs() > 16 * 2.0 ** -23 * max(float(h.double().pow(2).mean().sqrt()), 0.1)
        return (h >= 0).float(), keep
    return trajectory(c, x, i.v_th)[1], None


# ------------------------------------------------------------------ the fp64 reference under autograd
class ATanForced(torch.autograd.Function):
    """surrogate.ATan: backward alpha / 2 / (1 + (pi / 2 alpha u)^2) * g; forward heaviside(u), or the forced decision."""

    @staticmethod
    def forward(ctx, u, forced):
        ctx.save_for_backward(u)
        return (u >= 0).to(u.dtype) if forced is None else forced.to(u.dtype)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return ALPHA / 2 / (1 + (math.pi / 2 * ALPHA * u).pow(2)) * g, None


def _lif_loop(x, kind, tau, k, v_th, v_reset, detach, sltt, forced):
    """Multi-step LIF / IF / ParametricLIF (k: per-step leaves (T, ...)), SLTT with the membrane detached in the charge."""
    v = torch.zeros_like(x[0]) if v_reset is None else torch.full_like(x[0], v_reset)
    out = []
    for t in range(x.shape[0]):
        vc = v.detach() if sltt else v
        rest = vc if v_reset is None else vc - v_reset
        if kind == "if":
            h = vc + x[t]
        elif kind == "plif":
            h = vc + (x[t] - rest) * k[t]
        else:
            h = vc + (x[t] - rest) / tau
        s = ATanForced.apply(h - v_th, None if forced is None else forced[t])
        sr = s.detach() if detach else s
        v = h - sr * v_th if v_reset is None else (1.0 - sr) * h + sr * v_reset
        out.append(s)
    return torch.stack(out)


def _glif_loop(x, tab, forced):
    """GatedLIFNode.multi_step_forward on the derived table; tab: per-step leaves (T, 5 + T, N).  The spike is not detached."""
    v, s, out = torch.zeros_like(x[0]), torch.zeros_like(x[0]), []
    for t in range(x.shape[0]):
        L, Dk, gg, R, th, ct = tab[t, 0], tab[t, 1], tab[t, 2], tab[t, 3], tab[t, 4], tab[t, 5 + t]
        u = (L * v - Dk) + x[t] * ct
        u = u - L * v * gg * s - R * s
        s = ATanForced.apply(u - th, None if forced is None else forced[t])
        v = u
        out.append(s)
    return torch.stack(out)


Ref = namedtuple("Ref", "gx gk par par_abs gh")     # gx: dL/dx or dL/dq; gk: the gate's dL/dk; par / par_abs: name -> value, sum |terms|


@functools.lru_cache(4)
def reference(c, dtype=torch.float64, detach=None):
    """Gradients of the case from autograd through the per-step loop in `dtype`, decisions forced to the fp32 trajectory's."""
    return reference_on(c, inputs(c), decisions(c)[0], dtype, detach)


def reference_on(c, i, forced, dtype=torch.float64, detach=None):
    """The same on given inputs and decisions (the committed fixtures' own inputs); c names the neuron and its setting."""
    detach = c.detach if detach is None else detach
    d = lambda t: t.detach().to(dtype).clone()
    x = d(i.x).requires_grad_(True)
    vr, par, par_abs, gh, gk = RESETS[c.reset], {}, {}, None, None
    gate = c.family.startswith("gate_")
    xin = head_sums(x) if gate else x
    T, shp = xin.shape[0], tuple(xin.shape[1:])
    leaves = {}
    if c.family in ("psn", "gate_psn"):
        W = d(i.aux["W"]).reshape(T, T, *([1] * len(shp))).expand(T, T, *shp).clone().requires_grad_(True)
        b = d(i.aux["b"]).reshape(T, *([1] * len(shp))).expand(T, *shp).clone().requires_grad_(True)
        leaves = {"W": W, "b": b}
        h = torch.stack([b[t] + sum(W[t, k] * xin[k] for k in range(T)) for t in range(T)])      # addmm, one term per leaf
        h.retain_grad()
        s = ATanForced.apply(h, forced)
    elif c.family == "glif":
        tab = d(i.aux["tab"])[None, :, None].expand(T, 5 + T, *shp).clone().requires_grad_(True)
        leaves = {"tab": tab}
        s = _glif_loop(xin, tab, forced)
    else:
        kind, k = kind_of(c), None
        if kind == "plif":
            k = d(plif_k(c)).expand(T, *shp).clone().requires_grad_(True)
            leaves = {"k": k}
        s = _lif_loop(xin, kind, c.tau, k, i.v_th, vr, detach, c.family == "sltt", forced)
    if gate:
        kk = d(i.aux["k"]).requires_grad_(True)
        (kk * s.repeat_interleave(32, dim=-1)).backward(d(i.g))
        gk = kk.grad
    else:
        s.backward(d(i.g))
    if c.family in ("psn", "gate_psn"):
        red = tuple(range(2, 2 + len(shp)))
        par = {"W": leaves["W"].grad.sum(red), "b": leaves["b"].grad.sum(tuple(range(1, 1 + len(shp))))}
        par_abs = {"W": leaves["W"].grad.abs().sum(red), "b": leaves["b"].grad.abs().sum(tuple(range(1, 1 + len(shp))))}
        gh = h.grad
    elif c.family == "glif":
        par, par_abs = {"tab": leaves["tab"].grad.sum((0, 2))}, {"tab": leaves["tab"].grad.abs().sum((0, 2))}
    elif leaves:
        par, par_abs = {"k": leaves["k"].grad.sum()}, {"k": leaves["k"].grad.abs().sum()}
    return Ref(x.grad, gk, par, par_abs, gh)


def lif_backward(c):
    """oracle/neuron_bwd_ref.lif_backward on the case: what LIF / IF with a detached reset and a power-of-two tau are bit-equal to."""
    i = inputs(c)
    return BW.lif_backward(i.x, i.g, c.tau, i.v_th, RESETS[c.reset], c.detach, ALPHA, kind=kind_of(c))


def rel_dist(got, ref):
    """max |got - ref| relative to the largest element of the reference."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def gx_bound(c):
    """1e-6 of the largest element; at T = 16 and 20, max(1e-6, 4 x the distance of the SAME loop's fp32 autograd from its fp64 one) -
    the reference's own rounding on these inputs, the factor 4 for a different but legal summation order."""
    if c.T not in (16, 20):
        return 1e-6, 0.0
    own = rel_dist(reference(c, torch.float32).gx, reference(c).gx)
    return max(1e-6, 4 * own), own
