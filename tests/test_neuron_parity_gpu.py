"""Value parity of every instantiation of the stand-alone neuron kernels of the training path (csrc/neuron_bwd.hip, csrc/glif.hip,
csrc/qk_gate_train.hip, the PLIF training forward of csrc/neuron.hip) against an fp64 autograd reference with forced decisions.
Cases, inputs, references and the launch lines derived from the dispatch code: tests/neuron_train_cases.py.

GPU tests, one per (kernel family, T); every case of it
  * asserts its launches through hip.launch_log() against the enumeration (kernel<template arguments>, workgroups, 256 threads),
  * runs twice, bit-equal,
  * goes through the hip.* wrappers (the PSN backward with dL/dh at T <= 10 through the C ABI),
  * prints the measured distance and its bound, then asserts.
Sizes: N = 1028 (two workgroups, the second ragged), gate rows = 9 at C = 32 .. 768; one large case per reducing kernel at its
smallest T (257 partials for the finish kernels, a second ragged turn of the PSN grid-stride loop).

Bounds (from the project's own tests, not from the kernels):
  * forwards (sdf_plif_fwd, sdf_glif_fwd fp32 / u8, the gates' e) bit-equal to the fp32 trajectory; LIF / IF backward with a detached reset
    and tau = 2 bit-equal to oracle/neuron_bwd_ref.lif_backward at every T; the gate's dL/dk bit-equal to dL/de * A;
  * dL/dx, dL/dq, dL/dh within 1e-6 of the largest element of the fp64 reference; at T = 16, 20 within max(1e-6, 4 x the distance of the
    same loop's fp32 autograd from the fp64 one) - neuron_train_cases.gx_bound;
  * parameter gradients (dk, grad_tab, dW, db) within 1e-5 of the sum of the absolute values of the terms each sums;
  * PSN gate: W, b multiples of 2^-6 - e and dL/dk bit for bit; one random-W case per Tq under the 16-ulp rule, at most 1e-4 of the
    decisions left out (held on the CPU against the reference alone);
  * PSN backward at T <= 10: dL/dx of the reducing, the non-reducing and the dL/dh form bit-equal to each other.

The unmarked tests hold the premises without a GPU: the reference reproduces every committed fixture made by the real reference's
autograd at the bounds their GPU tests state, the enumeration covers the T lists and every instantiation the dispatch code can
produce, and the four overwritten column blocks do what they are for in the fp32 trajectory.

Measured on an MI355X (worst case per family over every T): dL/dx-type distances LIF 1.6e-7, IF 3.9e-7 (T = 20, bound 1.5e-6), SLTT 1.5e-7,
PLIF 1.9e-7, PSN 3.9e-7, GLIF 4.4e-7, gates 2.2e-7 of the largest element; parameter gradients at most 2.1e-7 of sum |terms|; the
random-W PSN gate cases leave out 0 of 501 / 1002 / 2004 decisions."""
import os

import numpy as np
import pytest
import torch

import neuron_train_cases as NC
from sdformerflow_amd import hip
from sdformerflow_amd.synthetic import synth_state_dict, synth_uniform as rnd

DEV = "cuda:0"
gpu = pytest.mark.gpu
GROUPS = NC.groups()


def of(*families):
    return [g for g in GROUPS if g[0] in families]


def dev(t):
    return t.to(DEV).contiguous()


def run2(call, expect):
    """call() under hip.launch_log(), twice: the launches are `expect` = ((kernel name part, workgroups), ...) on 256 threads and the
    two results are bit-equal; the first result (a tensor or a tuple of tensors / None)."""
    outs = []
    for _ in range(2):
        with hip.launch_log() as log:
            out = call()
        torch.cuda.synchronize()
        assert len(log.rows) == len(expect), (log.rows, expect)
        for (kname, wgs, threads, _, _), (part, want) in zip(log.rows, expect):
            assert part in kname and wgs == want and threads == 256, (kname, wgs, threads, part, want)
        outs.append(out if isinstance(out, tuple) else (out,))
    for a, b in zip(*outs):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                        b.view(torch.int32) if b.dtype == torch.float32 else b), "two calls differ"
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def held(c, what, got, ref, bound, note=""):
    """Print, then assert: max |got - ref| relative to the largest element of ref within `bound`."""
    dist = NC.rel_dist(got.cpu(), ref)
    print(f"PARITY {NC.name(c)} {what}: distance {dist:.3e} bound {bound:.3e}{note}")
    assert dist <= bound, (NC.name(c), what, dist, bound)


def held_sum(c, what, got, ref, ref_abs):
    """Print, then assert: a reduced gradient within 1e-5 of the sum of the absolute values of its terms, entry by entry."""
    d = (got.cpu().double().reshape(ref.shape) - ref).abs()
    worst = float((d / ref_abs.clamp_min(1e-300)).max())
    print(f"PARITY {NC.name(c)} {what}: distance/sum|terms| {worst:.3e} bound 1.000e-05")
    assert bool((d <= 1e-5 * ref_abs).all()), (NC.name(c), what, d, ref_abs)
    assert bool((got != 0).any())


def every(cases, one):
    """one(c) for every case; the failures of all of them in one assertion."""
    failed = []
    for c in cases:
        try:
            one(c)
        except AssertionError as e:
            failed.append(f"{NC.name(c)}: {(str(e).splitlines() or ['not bit-equal'])[0]}")
    assert not failed, f"{len(failed)} of {len(cases)} cases: " + "; ".join(failed)


def gx_bound(c):
    bound, own = NC.gx_bound(c)
    return bound, f" (fp32 autograd of the same loop: {own:.3e})" if own else ""


# ------------------------------------------------------------------ GPU: LIF / IF / SLTT / PLIF
@gpu
@pytest.mark.parametrize("family,T", of("lif", "if", "sltt"))
def test_lif_family_backward(family, T):
    def one(c):
        i, vr = NC.inputs(c), NC.RESETS[c.reset]
        x, g = dev(i.x), dev(i.g)
        if family == "sltt":
            gx = run2(lambda: hip.sltt_bwd(x, g, c.tau, i.v_th, vr, NC.ALPHA), c.launches)
        else:
            gx = run2(lambda: hip.lif_bwd(x, g, c.tau, i.v_th, vr, c.detach, NC.ALPHA, kind=family), c.launches)
        bound, note = gx_bound(c)
        held(c, "gx", gx, NC.reference(c).gx, bound, note)
        if family == "sltt":                                           # the reset only feeds the detached membrane
            held(c, "gx(reference not detached)", gx, NC.reference(c, detach=False).gx, bound)
        elif c.detach and c.tau == 2.0:
            assert torch.equal(gx.cpu(), NC.lif_backward(c)), NC.name(c)

    every(NC.cases_of(family, T), one)


@gpu
@pytest.mark.parametrize("family,T", of("plif"))
def test_plif_forward_and_backward(family, T):
    def one(c):
        i, vr = NC.inputs(c), NC.RESETS[c.reset]
        x, g, k = dev(i.x), dev(i.g), dev(NC.plif_k(c).reshape(1))
        s = run2(lambda: hip.plif_fwd(x, k, i.v_th, vr), c.fwd_launches)
        assert torch.equal(s.cpu(), NC.decisions(c)[0]), NC.name(c)
        gx, gk = run2(lambda: hip.plif_bwd(x, k, g, i.v_th, vr, c.detach, NC.ALPHA), c.launches)
        ref = NC.reference(c)
        bound, note = gx_bound(c)
        held(c, "gx", gx, ref.gx, bound, note)
        held_sum(c, "dk", gk, ref.par["k"], ref.par_abs["k"])

    every(NC.cases_of(family, T), one)


# ------------------------------------------------------------------ GPU: PSN
def psn_bwd_abi(x, W, b, g, want_gh):
    """sdf_psn_bwd with grad_W == NULL through the C ABI: (dL/dx, dL/dh or None)."""
    T, N = x.shape
    gx, gh = torch.empty_like(x), torch.empty_like(x) if want_gh else None
    rc = hip.lib().sdf_psn_bwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), g.data_ptr(), gx.data_ptr(), None, None,
                               gh.data_ptr() if want_gh else None, None, 0, T, N, 0, NC.ALPHA, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return gx, gh


@gpu
@pytest.mark.parametrize("family,T", of("psn"))
def test_psn_backward(family, T):
    def one(c):
        i = NC.inputs(c)
        x, g, W, b = dev(i.x), dev(i.g), dev(i.aux["W"]), dev(i.aux["b"])
        ref = NC.reference(c)
        bound, note = gx_bound(c)
        gx_n, _ = run2(lambda: psn_bwd_abi(x, W, b, g, False), c.launches)
        gx_h, gh = run2(lambda: psn_bwd_abi(x, W, b, g, True), c.launches)
        assert torch.equal(gx_n, gx_h), NC.name(c)
        assert torch.equal(run2(lambda: hip.psn_bwd(x, W, b, g, NC.ALPHA, need_param_grads=False)[0], c.launches), gx_n)
        if c.fwd_launches:                                              # the reducing kernel and its finish
            gx, gW, gb = run2(lambda: hip.psn_bwd(x, W, b, g, NC.ALPHA), c.fwd_launches)
            assert torch.equal(gx, gx_n), NC.name(c)                    # the same per-element arithmetic in all three forms
        else:                                                           # T > 10: dL/dh from the kernel, one library GEMM
            with hip.launch_log() as log:
                gx, gW, gb = hip.psn_bwd(x, W, b, g, NC.ALPHA)
            assert [r[1] for r in log.rows] == [w for _, w in c.launches] and c.launches[0][0] in log.rows[0][0]
            assert torch.equal(gx, gx_n), NC.name(c)
        held(c, "gx", gx_n, ref.gx, bound, note)
        held(c, "gh", gh, ref.gh, bound, note)
        held_sum(c, "dW", gW, ref.par["W"], ref.par_abs["W"])
        held_sum(c, "db", gb, ref.par["b"], ref.par_abs["b"])

    every(NC.cases_of(family, T), one)


# ------------------------------------------------------------------ GPU: GLIF
@gpu
@pytest.mark.parametrize("family,T", of("glif"))
def test_glif_forward_and_backward(family, T):
    def one(c):
        i = NC.inputs(c)
        x, g, tab = dev(i.x), dev(i.g), dev(i.aux["tab"])
        want = NC.decisions(c)[0]
        s32 = run2(lambda: hip.glif_fwd(x, tab), c.fwd_launches[:1])
        s8 = run2(lambda: hip.glif_fwd(x, tab, torch.uint8), c.fwd_launches[1:])
        assert torch.equal(s32.cpu(), want) and torch.equal(s8.cpu(), want.to(torch.uint8)), NC.name(c)
        gx, gtab = run2(lambda: hip.glif_bwd(x, tab, g, NC.ALPHA), c.launches)
        ref = NC.reference(c)
        bound, note = gx_bound(c)
        held(c, "gx", gx, ref.gx, bound, note)
        held_sum(c, "grad_tab", gtab, ref.par["tab"], ref.par_abs["tab"])

    every(NC.cases_of(family, T), one)


# ------------------------------------------------------------------ GPU: the token gate
@gpu
@pytest.mark.parametrize("family,Tq", of("gate_lif", "gate_if", "gate_plif"))
def test_gate_lif_if_plif(family, Tq):
    def one(c):
        i, vr = NC.inputs(c), NC.RESETS[c.reset]
        q, k, ge = dev(i.x), dev(i.aux["k"]), dev(i.g)
        A = NC.decisions(c)[0].repeat_interleave(32, dim=-1)
        if family == "gate_plif":
            pk = dev(NC.plif_k(c).reshape(1))
            e = run2(lambda: hip.qk_gate_plif_f32(q, k, pk, i.v_th, vr), c.fwd_launches)
            gq, gk, gpk = run2(lambda: hip.qk_gate_plif_bwd(q, k, ge, pk, i.v_th, vr, c.detach, NC.ALPHA), c.launches)
        else:
            p = hip.NeuronParams(NC.kind_of(c), c.tau, i.v_th, vr)
            e = run2(lambda: hip.qk_gate_f32(q, k, p), c.fwd_launches)
            gq, gk, gW, gb = run2(lambda: hip.qk_gate_bwd(q, k, ge, p, c.detach, NC.ALPHA), c.launches)
            assert gW is None and gb is None
        assert torch.equal(e.cpu(), i.aux["k"] * A), NC.name(c)
        assert torch.equal(gk.cpu(), i.g * A), NC.name(c)
        ref = NC.reference(c)
        held(c, "gq", gq, ref.gx, 1e-6)
        held(c, "gk", gk, ref.gk, 1e-6)
        if family == "gate_plif":
            held_sum(c, "dk", gpk, ref.par["k"], ref.par_abs["k"])

    every(NC.cases_of(family, Tq), one)


@gpu
@pytest.mark.parametrize("family,Tq", of("gate_psn"))
def test_gate_psn(family, Tq):
    def one(c):
        i = NC.inputs(c)
        q, k, ge = dev(i.x), dev(i.aux["k"]), dev(i.g)
        p = hip.NeuronParams("psn", psn_w=dev(i.aux["W"]), psn_b=dev(i.aux["b"]))
        A, keep = NC.decisions(c)
        e = run2(lambda: hip.qk_gate_f32(q, k, p), c.fwd_launches)
        gq, gk, gW, gb = run2(lambda: hip.qk_gate_bwd(q, k, ge, p, True, NC.ALPHA), c.launches)
        A = A.repeat_interleave(32, dim=-1)
        if dict(c.kw)["W"] == "exact":                                  # every partial sum exact in fp32: bit for bit
            assert torch.equal(e.cpu(), i.aux["k"] * A) and torch.equal(gk.cpu(), i.g * A), NC.name(c)
        else:                                                           # the 16-ulp rule
            m = keep.repeat_interleave(32, dim=-1)
            print(f"PARITY {NC.name(c)} left out: {float((~keep).float().mean()):.3e} of {keep.numel()} decisions")
            assert torch.equal(e.cpu()[m], (i.aux["k"] * A)[m]) and torch.equal(gk.cpu()[m], (i.g * A)[m]), NC.name(c)
        ref = NC.reference(c)
        held(c, "gq", gq, ref.gx, 1e-6)
        if dict(c.kw)["W"] == "exact":
            held(c, "gk", gk, ref.gk, 1e-6)
        held_sum(c, "dW", gW, ref.par["W"], ref.par_abs["W"])
        held_sum(c, "db", gb, ref.par["b"], ref.par_abs["b"])

    every(NC.cases_of(family, Tq), one)


# ------------------------------------------------------------------ CPU: the premises
def load(name):
    return np.load(os.path.join(NC.GOLD, name + ".npz"))


def fixture_case(family, T, x, g, v_th, reset="soft", detach=True, tau=2.0, kw=None, aux=None):
    c = NC._case(family, T, N=x[0].numel(), reset=reset, detach=detach, tau=tau, kw=kw)
    return c, NC.Inputs(x.reshape(T, -1), g.reshape(T, -1), v_th, aux or {})


def fixture_inputs(T, n, seed_x, seed_g, tie_x):
    x = rnd((T, n), seed_x, -0.3, 0.6)
    x[:, :64] = 0.1
    x[0, 64:128] = tie_x
    return x, rnd((T, n), seed_g, -1.0, 2.0)


@pytest.mark.parametrize("T", [2, 10])
def test_reference_reproduces_the_lif_and_psn_fixtures(T):
    """neuron_grads.npz at the bounds of test_hip_kernels.py: LIF bit-equal (the fp32 run of the same loop) when the reset is detached and
    tau = 2, 1e-6 of the largest element otherwise and for the fp64 run throughout; PSN 1e-5 of the largest element."""
    NG = load("neuron_grads")
    x, g = fixture_inputs(T, 2048, 300 + T, 400 + T, 0.2)
    for tag, reset, detach, tau in (("soft_detach", "soft", True, 2.0), ("soft_nodetach", "soft", False, 2.0), ("hard_detach", "hard", True, 2.0),
                                    ("hard_nodetach", "hard", False, 2.0), ("tau3_soft_detach", "soft", True, 3.0)):
        c, i = fixture_case("lif", T, x, g, 0.1, reset, detach, tau)
        h, s = NC.trajectory(c, x, 0.1)
        assert np.array_equal(s.numpy().astype(np.uint8), NG[f"lif_{tag}_T{T}_s"])
        assert int((h[0, 64:128] - 0.1 == 0).sum()) == 64 or tau != 2.0
        want = torch.from_numpy(NG[f"lif_{tag}_T{T}_gx"])
        assert NC.rel_dist(NC.reference_on(c, i, s).gx, want) <= 1e-6, tag
        got32 = NC.reference_on(c, i, s, torch.float32).gx
        if detach and tau == 2.0:
            assert torch.equal(got32, want), tag
        else:
            assert NC.rel_dist(got32, want) <= 1e-6, tag
    sd = synth_state_dict({"spiking_neuron.weight": (T, T), "spiking_neuron.bias": (T, 1)}, salt=T)
    c, i = fixture_case("psn", T, x, g, 0.0, aux={"W": sd["spiking_neuron.weight"], "b": sd["spiking_neuron.bias"].reshape(T)})
    r = NC.reference_on(c, i, None)
    for got, key in ((r.gx, "gx"), (r.par["W"], "gW"), (r.par["b"], "gb")):
        assert NC.rel_dist(got.reshape(-1), torch.from_numpy(NG[f"psn_T{T}_{key}"]).reshape(-1)) <= 1e-5, key


@pytest.mark.parametrize("T", [2, 4, 10])
def test_reference_reproduces_the_plif_and_sltt_fixtures(T):
    """plif_grads.npz and sltt_grads.npz at the bounds of test_plif_train_gpu.py / test_glif_sltt_train_gpu.py: spikes equal, dL/dx within
    1e-6 of the largest element, dL/dw within 1e-5 of sum |gh d| carried to w."""
    PG, SG = load("plif_grads"), load("sltt_grads")
    k = float(NC.plif_k(NC._case("plif", T, kw={"k": "k035"})))
    assert float(PG["w"]) == np.float32(NC.PLIF_KS["k035"])
    for tag in NC.RESETS:
        for detach in (True, False):
            key = f"{tag}_{'detach' if detach else 'nodetach'}_T{T}"
            x, g = fixture_inputs(T, 256, 500 + T, 600 + T, float(PG[f"{tag}_T{T}_tie_x"]))
            c, i = fixture_case("plif", T, x, g, float(PG["v_th"]), tag, detach, kw={"k": "k035"})
            h, s = NC.trajectory(c, x, i.v_th)
            assert np.array_equal(s.numpy().astype(np.uint8), PG[f"{key}_s"]) and int((h[0, 64:128] - i.v_th == 0).sum()) == 64
            r = NC.reference_on(c, i, s)
            assert NC.rel_dist(r.gx, torch.from_numpy(PG[f"{key}_gx"])) <= 1e-6, key
            to_w = k * (1 - k)
            assert abs(float(r.par["k"]) * to_w - float(PG[f"{key}_gw"])) <= 1e-5 * float(r.par_abs["k"]) * to_w, key
            x, g = fixture_inputs(T, 256, 1200 + T, 1300 + T, float(SG[f"{tag}_T{T}_tie_x"]))
            c, i = fixture_case("sltt", T, x, g, float(SG["v_th"]), tag, detach)
            h, s = NC.trajectory(c, x, i.v_th)
            assert np.array_equal(s.numpy().astype(np.uint8), SG[f"{key}_s"]) and int((h[0, 64:128] - i.v_th == 0).sum()) == 64
            assert NC.rel_dist(NC.reference_on(c, i, s).gx, torch.from_numpy(SG[f"{key}_gx"])) <= 1e-6, key


@pytest.mark.parametrize("T", [2, 4, 10])
def test_reference_reproduces_the_glif_fixture(T):
    """glif_grads.npz at the bounds of test_glif_sltt_train_gpu.py: spikes equal, dL/dx within 1e-6 of the largest element, grad_tab within
    1e-5 of the sum of the absolute values of its terms of the generator's fp64 evaluation (`gtab64`, `gtab_abs`); the reference's own
    sum |terms| is that sum to 1e-6 of it."""
    GG = load("glif_grads")
    tab, sd, tie_x = NC.glif_table(T)
    for si, (tag, n) in enumerate((("N256", 256), ("N105", 105), ("N3076", 3076))):
        blk = 64 if n >= 256 else 8
        x = 3.0 * rnd((T, n), 1000 + 10 * T + si, -0.3, 0.6)
        x[0, :blk], x[:, blk:2 * blk] = tie_x, 2.5
        g = rnd((T, n), 1100 + 10 * T + si, -1.0, 2.0)
        c, i = fixture_case("glif", T, x, g, float(tab[4]), aux={"tab": tab, "sd": sd})
        s = NC.O.glif_multistep(x, sd, "spiking_neuron.")
        assert np.array_equal(s.numpy().astype(np.uint8).reshape(-1), GG[f"T{T}_{tag}_s"].reshape(-1))
        r = NC.reference_on(c, i, s)
        assert NC.rel_dist(r.gx.reshape(-1), torch.from_numpy(GG[f"T{T}_{tag}_gx"]).reshape(-1)) <= 1e-6, tag
        gt64, gabs = torch.from_numpy(GG[f"T{T}_{tag}_gtab64"]), torch.from_numpy(GG[f"T{T}_{tag}_gtab_abs"])
        assert bool(((r.par["tab"] - gt64).abs() <= 1e-5 * gabs).all()), tag
        assert bool(((r.par_abs["tab"] - gabs).abs() <= 1e-6 * gabs).all()), tag      # (its u_t are the fp32 ones, 6e-8 from these)


def test_enumeration_covers_the_t_lists_and_every_instantiation():
    L = NC.t_lists()
    assert all(len(v) == len(set(v)) and v == tuple(sorted(v)) for v in L.values())
    for fam in NC.STREAM_FAMILIES:
        assert tuple(T for f, T in GROUPS if f == fam) == L["STREAM"]
    assert tuple(T for f, T in GROUPS if f == "glif") == L["GLIF"]
    for fam in NC.GATE_FAMILIES:
        assert tuple(T for f, T in GROUPS if f == fam) == L["GATE"]
    cases = NC.all_cases()
    assert len({NC.name(c) for c in cases}) == len(cases)
    named = {part for c in cases for part, _ in c.launches + c.fwd_launches}
    assert named == NC.instantiations() and len(named) == 65 + 3
    reduce_t = [T for T in L["STREAM"] if NC.psn_reduce_vec(T)]
    assert min(T for T in reduce_t if NC.psn_reduce_vec(T) == 2) == 8 and max(reduce_t) == 10
    # the large cases do reach the second turns they are for
    big = {(c.family, c.T): c for c in cases if max(c.N, c.rows) > 4096 and c.family != "psn"}
    assert set(big) == {("plif", 1), ("glif", 2), ("gate_plif", 1), ("gate_psn", 1)}
    assert all(c.launches[0][1] == 257 for c in big.values())
    psn_big = {c.T: c for c in cases if c.family == "psn" and c.N > 4096}
    assert set(psn_big) == {2, 8}
    for T, c in psn_big.items():
        vec = NC.psn_reduce_vec(T)
        assert c.fwd_launches[0][1] == 512 and c.N // vec > 512 * 256 and (c.N // vec) % 256 != 0 and c.N % 4 == 0
    assert all(c.T * max(c.N, c.rows * c.C) * 4 <= 10 << 20 for c in cases)                   # nothing above 10 MB per tensor
    for c in cases:
        assert c.N % 4 == 0 and c.C % 32 == 0


@pytest.mark.parametrize("family,T", [g for g in GROUPS if g[0] not in ("psn", "gate_psn")])
def test_the_four_column_blocks_do_what_they_are_for(family, T):
    """In the fp32 trajectory of every case: the tie block holds h_0 - v_th == 0 exactly (and fires), the hard block fires at every
    step, the silent block never, the late block at the last step only.  dL/ds of a `wide` case spans six decades."""
    for c in NC.cases_of(family, T):
        i = NC.inputs(c)
        s = NC.decisions(c)[0]
        if family == "glif":
            tab, b = i.aux["tab"], NC.blocks(c.N)
            u0 = ((torch.zeros(()) - tab[1]) + i.x[0, b["tie"]] * tab[5]) - tab[4]
            s = s.reshape(T, -1)
        elif family.startswith("gate_"):
            sums = NC.head_sums(i.x).reshape(T, -1)
            assert sums[:, :4].t().tolist() == [[float(NC.GATE_TIE)] * T, [32.0] * T, [0.0] * T, [0.0] * (T - 1) + [32.0]]
            b = {k: slice(n, n + 1) for n, k in enumerate(("tie", "hard", "silent", "late"))}
            u0 = NC.trajectory(c, sums, i.v_th)[0][0, b["tie"]] - i.v_th
            s = s.reshape(T, -1)
        else:
            b = NC.blocks(c.N)
            u0 = NC.trajectory(c, i.x, i.v_th)[0][0, b["tie"]] - i.v_th
        assert bool((u0 == 0).all()) and bool((s[0, b["tie"]] == 1).all()), NC.name(c)
        assert bool((s[:, b["hard"]] == 1).all()) and not bool(s[:, b["silent"]].any()), NC.name(c)
        assert bool((s[T - 1, b["late"]] == 1).all()) and not bool(s[:T - 1, b["late"]].any()), NC.name(c)
        assert 0.02 < float(s.mean()) < 0.98
        if c.wide:
            assert float(i.g.abs().max() / i.g.abs().min()) > 1e5


@pytest.mark.parametrize("Tq", NC.t_lists()["GATE"])
def test_psn_gate_decisions_of_the_reference_alone(Tq):
    """Exact weights: h of the fp32 chain equals the fp64 h bit for bit, no decision near 0 matters.  Random weights under the 16-ulp
    rule: every decision kept agrees with the fp64 evaluation and at most 1e-4 of them are left out."""
    for c in NC.cases_of("gate_psn", Tq):
        i = NC.inputs(c)
        sums, W, b = NC.head_sums(i.x).double(), i.aux["W"].double(), i.aux["b"].double()
        h64 = b.reshape(Tq, 1, 1) + torch.einsum("tk,krg->trg", W, sums)
        A, keep = NC.decisions(c)
        assert 0.02 < float(A.mean()) < 0.98, NC.name(c)
        if dict(c.kw)["W"] == "exact":
            assert bool((W * 64 == torch.round(W * 64)).all()) and float(W.abs().max()) < 1 and bool((b * 64 == torch.round(b * 64)).all())
            assert torch.equal(NC.psn_gate_h32(sums.float(), i.aux["W"], i.aux["b"]).double(), h64)
        else:
            assert bool(((h64 >= 0).float() == A)[keep].all())
            assert float((~keep).float().mean()) <= 1e-4, NC.name(c)
