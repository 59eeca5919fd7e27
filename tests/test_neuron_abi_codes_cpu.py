"""Return codes of the stand-alone neuron entry points, pinned one fault at a time: the host side of neuron.hip, neuron_bwd.hip,
glif.hip and qk_gate_train.hip checks its arguments in a fixed order and answers with a fixed code before any launch, so dummy
device pointers do and no GPU is needed.  Every vector starts from a valid call (T = 10, N = 4096; gate: Tq = 2, rows = 64, C = 96)
and breaks one argument - or two, where the ORDER of the checks decides the answer.  Only faults that are refused are listed: a
(T, N) that merely takes another kernel (sdf_lif_fwd / sdf_psn_fwd with N % 4 != 0, an unlisted T of sdf_neuron_fwd) would launch.
The expected codes are those the library returned before csrc/host_launch.h stated the T sets and the dispatch once."""
import ctypes as C
import os

import pytest

P, ODD16, ODD4 = 0x10000, 0x10004, 0x10002          # aligned; not 16-byte aligned; not 4-byte aligned
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
T_STREAM, T_GLIF, T_GATE = (1, 2, 4, 5, 8, 10, 16, 20), (2, 4, 5, 10, 20), (1, 2, 4)
T_BAD = (0, 3, 7, 12, 40)                           # just outside and between the legal values of every list
BIG = 1 << 20


@pytest.fixture(scope="module")
def lib():
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


def entry(fn, order, **base):
    """call(**overrides) -> return code of `fn` with the baseline arguments `base`, passed in `order`."""
    def call(**kw):
        unknown = set(kw) - set(base)
        assert not unknown, unknown
        a = dict(base, **kw)
        return fn(*[a[n] for n in order.split()])
    return call


def run(call, vectors):
    for kw, want in vectors:
        got = call(**kw)
        assert got < 0, ("reached a launch", kw, got)
        assert got == want, (kw, got, want)


def each(names, value, want):
    return [({n: value}, want) for n in names.split()]


def desc(**kw):
    from sdformerflow_amd import hip
    d = hip.NeuronDesc()
    base = dict(x=P, out=P, T=10, out_dtype=0, nb=1, ni=4096, x_sb=0, x_st=4096, o_sb=0, o_st=4096, kind=0, tau=2.0, v_th=0.1,
                soft_reset=1)
    for f, v in dict(base, **kw).items():
        setattr(d, f, v)
    return d


def test_lif_fwd_and_psn_fwd(lib):
    lif = entry(lib.sdf_lif_fwd, "x s v T N tau vth soft vr dt st", x=P, s=P, v=None, T=10, N=4096, tau=2.0, vth=0.1, soft=1, vr=0.0,
                dt=0, st=None)
    run(lif, each("x s", None, E_NULL) + each("x s v", ODD16, E_ALIGN) + [
        ({"T": 0}, E_SHAPE), ({"N": 0}, E_SHAPE), ({"dt": 2}, E_DTYPE), ({"tau": 1.0}, E_SHAPE), ({"tau": 0.0}, E_SHAPE),
        ({"dt": 1, "s": ODD4}, E_ALIGN),
        ({"x": None, "T": 0}, E_NULL), ({"dt": 2, "x": ODD16}, E_DTYPE), ({"x": ODD16, "tau": 1.0}, E_ALIGN),
        ({"v": ODD16, "tau": 1.0}, E_SHAPE)])
    psn = entry(lib.sdf_psn_fwd, "x W b s T N dt st", x=P, W=P, b=P, s=P, T=10, N=4096, dt=0, st=None)
    run(psn, each("x W b s", None, E_NULL) + each("x s", ODD16, E_ALIGN) + [
        ({"T": 0}, E_SHAPE), ({"N": 0}, E_SHAPE), ({"dt": 2}, E_DTYPE), ({"dt": 1, "s": ODD4}, E_ALIGN),
        ({"W": None, "x": ODD16}, E_ALIGN), ({"x": None, "dt": 2}, E_NULL)])


def test_neuron_fwd_and_multi_fwd(lib):
    one = lambda **kw: lib.sdf_neuron_fwd(C.byref(desc(**kw)), None)
    vectors = each("x out", None, E_NULL) + each("x out v_last", ODD16, E_ALIGN) + [
        ({"T": 0}, E_SHAPE), ({"ni": 0}, E_SHAPE), ({"ni": 4094}, E_SHAPE), ({"nb": 0}, E_SHAPE), ({"out_dtype": 2}, E_DTYPE),
        ({"kind": 3}, E_DTYPE), ({"tau": 1.0}, E_SHAPE), ({"out_dtype": 1, "out": ODD4}, E_ALIGN),
        ({"x_st": 4094}, E_SHAPE), ({"o_st": 4094}, E_SHAPE), ({"nrep": -1}, E_SHAPE), ({"nrep": 2, "x_srep": 6}, E_SHAPE),
        ({"rowmap": P, "rowlen": 0}, E_SHAPE), ({"alpha": P}, E_NULL), ({"alpha": P, "beta": P, "C": 0, "inner": 1}, E_SHAPE),
        ({"alpha": ODD16, "beta": P, "C": 4, "inner": 1}, E_ALIGN), ({"add": P, "add_period": 0}, E_SHAPE),
        ({"kind": 1}, E_NULL), ({"kind": 1, "psn_w": P, "psn_b": P, "v_last": P}, E_SHAPE),
        ({"x": None, "T": 0}, E_NULL), ({"out_dtype": 2, "x": ODD16}, E_DTYPE), ({"ni": 4094, "x": ODD16}, E_SHAPE),
        ({"x": ODD16, "tau": 1.0}, E_ALIGN), ({"v_last": ODD16, "tau": 1.0}, E_SHAPE)]
    for kw, want in vectors:
        assert one(**kw) == want, kw
    assert lib.sdf_neuron_fwd(None, None) == E_NULL
    assert one(kind=1, psn_w=P, psn_b=P, T=3) == E_SHAPE                 # PSN has no runtime-T kernel (refused by the dispatch)

    from sdformerflow_amd import hip
    multi = lambda n, *ds: lib.sdf_neuron_multi_fwd((hip.NeuronDesc * max(len(ds), 1))(*ds), n, None)
    assert lib.sdf_neuron_multi_fwd(None, 2, None) == E_NULL
    assert multi(0, desc(), desc()) == E_SHAPE
    for kw, want in vectors:
        assert multi(1, desc(**kw)) == want, kw                          # n = 1 is sdf_neuron_fwd
        assert multi(2, desc(), desc(**kw)) == want, kw                  # every descriptor is validated before the first launch
        assert multi(7, *([desc()] * 6 + [desc(**kw)])) == want, kw      # ... also where there is one launch per descriptor
    assert multi(2, desc(T=0), desc(T=0)) == E_SHAPE
    assert multi(2, desc(ni=0), desc(x=None)) == E_SHAPE                 # the first faulty descriptor answers


def test_lif_bwd_and_sltt_bwd(lib):
    lif = entry(lib.sdf_lif_bwd, "x gs gx T N kind tau vth soft vr det sur alpha st", x=P, gs=P, gx=P, T=10, N=4096, kind=0, tau=2.0,
                vth=0.1, soft=1, vr=0.0, det=1, sur=0, alpha=2.0, st=None)
    run(lif, each("x gs gx", None, E_NULL) + each("x gs gx", ODD16, E_ALIGN) + [({"T": T}, E_SHAPE) for T in T_BAD] + [
        ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"kind": 1}, E_DTYPE), ({"kind": 3}, E_DTYPE), ({"sur": 1}, E_DTYPE),
        ({"tau": 0.5}, E_SHAPE), ({"tau": 1.0}, E_SHAPE), ({"kind": 2, "tau": 1.0, "T": 3}, E_SHAPE),
        ({"x": None, "T": 3}, E_NULL), ({"sur": 1, "gs": ODD16}, E_DTYPE), ({"kind": 3, "N": 4094}, E_SHAPE),
        ({"sur": 1, "tau": 1.0}, E_DTYPE), ({"T": 3, "gx": ODD16}, E_ALIGN)])          # T is checked last: by the dispatch
    sltt = entry(lib.sdf_sltt_bwd, "x gs gx T N tau vth soft vr sur alpha st", x=P, gs=P, gx=P, T=10, N=4096, tau=2.0, vth=0.1,
                 soft=1, vr=0.0, sur=0, alpha=2.0, st=None)
    run(sltt, each("x gs gx", None, E_NULL) + each("x gs gx", ODD16, E_ALIGN) + [({"T": T}, E_SHAPE) for T in T_BAD] + [
        ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"sur": 1}, E_SHAPE), ({"tau": 0.5}, E_SHAPE), ({"tau": 1.0}, E_SHAPE),
        ({"x": None, "T": 3}, E_NULL), ({"sur": 1, "gs": ODD16}, E_SHAPE), ({"T": 3, "gx": ODD16}, E_SHAPE)])   # T before alignment


def test_psn_bwd(lib):
    psn = entry(lib.sdf_psn_bwd, "x W b gs gx gW gb gh ws wsb T N sur alpha st", x=P, W=P, b=P, gs=P, gx=P, gW=P, gb=P, gh=None, ws=P,
                wsb=BIG, T=10, N=4096, sur=0, alpha=2.0, st=None)
    need = lib.sdf_psn_bwd_workspace_bytes(10, 4096)
    assert need == 8 * 110 * 4
    run(psn, each("x W b gs gx gb ws", None, E_NULL) + each("x gs gx gh", ODD16, E_ALIGN) + [({"T": T}, E_SHAPE) for T in T_BAD] + [
        ({"T": T, "gW": None, "gb": None, "ws": None, "wsb": 0}, E_SHAPE) for T in T_BAD] + [
        ({"T": 16}, E_SHAPE), ({"T": 20}, E_SHAPE),                      # no in-kernel dW / db reduction above T = 10
        ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"sur": 1}, E_DTYPE), ({"wsb": need - 1}, E_SHAPE),
        ({"x": None, "T": 3}, E_NULL), ({"sur": 1, "gs": ODD16}, E_DTYPE), ({"wsb": need - 1, "gx": ODD16}, E_ALIGN),
        ({"gb": None, "gx": ODD16}, E_ALIGN), ({"gb": None, "T": 12}, E_NULL), ({"T": 12, "wsb": 0}, E_SHAPE)])


def test_plif_fwd_and_bwd(lib):
    fwd = entry(lib.sdf_plif_fwd, "x k s T N vth soft vr st", x=P, k=P, s=P, T=10, N=4096, vth=0.1, soft=1, vr=0.0, st=None)
    run(fwd, each("x k s", None, E_NULL) + each("x s", ODD16, E_ALIGN) + [({"T": T}, E_SHAPE) for T in T_BAD] + [
        ({"k": ODD4}, E_ALIGN), ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE),
        ({"x": None, "T": 3}, E_NULL), ({"N": 4094, "x": ODD16}, E_SHAPE), ({"T": 3, "s": ODD16}, E_ALIGN)])   # T last: the dispatch
    bwd = entry(lib.sdf_plif_bwd, "x k gs gx gk ws wsb T N vth soft vr det sur alpha st", x=P, k=P, gs=P, gx=P, gk=P, ws=P, wsb=BIG,
                T=10, N=4096, vth=0.1, soft=1, vr=0.0, det=1, sur=0, alpha=2.0, st=None)
    need = lib.sdf_plif_bwd_workspace_bytes(10, 4096)
    assert need == 4 * 4
    run(bwd, each("x k gs gx gk ws", None, E_NULL) + each("x gs gx", ODD16, E_ALIGN) + each("k gk ws", ODD4, E_ALIGN) + [
        ({"T": T}, E_SHAPE) for T in T_BAD] + [
        ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"sur": 1}, E_DTYPE), ({"wsb": need - 1}, E_SHAPE),
        ({"ws": None, "T": 3}, E_NULL), ({"sur": 1, "T": 3}, E_DTYPE), ({"sur": 1, "N": 4094}, E_SHAPE),
        ({"T": 3, "gx": ODD16}, E_SHAPE), ({"wsb": need - 1, "gx": ODD16}, E_SHAPE), ({"sur": 1, "ws": ODD4}, E_DTYPE)])


def test_glif_fwd_and_bwd(lib):
    t_bad = T_BAD + (1, 8, 16)                                           # legal for the streaming kernels, not for GLIF
    fwd = entry(lib.sdf_glif_fwd, "x tab s T N dt st", x=P, tab=P, s=P, T=10, N=4096, dt=0, st=None)
    run(fwd, each("x tab s", None, E_NULL) + each("x s", ODD16, E_ALIGN) + [({"T": T}, E_SHAPE) for T in t_bad] + [
        ({"tab": ODD4}, E_ALIGN), ({"dt": 1, "s": ODD4}, E_ALIGN), ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"dt": 2}, E_DTYPE),
        ({"x": None, "T": 3}, E_NULL), ({"T": 3, "dt": 2}, E_SHAPE), ({"dt": 2, "x": ODD16}, E_DTYPE), ({"T": 3, "x": ODD16}, E_SHAPE)])
    bwd = entry(lib.sdf_glif_bwd, "x tab gs gx gt ws wsb T N sur alpha st", x=P, tab=P, gs=P, gx=P, gt=P, ws=P, wsb=BIG, T=10, N=4096,
                sur=0, alpha=2.0, st=None)
    need = lib.sdf_glif_bwd_workspace_bytes(10, 4096)
    assert need == 4 * 15 * 4
    run(bwd, each("x tab gs gx gt ws", None, E_NULL) + each("x gs gx", ODD16, E_ALIGN) + each("tab gt ws", ODD4, E_ALIGN) + [
        ({"T": T}, E_SHAPE) for T in t_bad] + [
        ({"N": 0}, E_SHAPE), ({"N": 4094}, E_SHAPE), ({"sur": 1}, E_SHAPE), ({"wsb": need - 1}, E_SHAPE),
        ({"ws": None, "T": 3}, E_NULL), ({"sur": 1, "gx": ODD16}, E_SHAPE), ({"wsb": need - 1, "gx": ODD16}, E_SHAPE)])


def test_qk_gate_train(lib):
    geo = [({"rows": 0}, E_SHAPE), ({"C": 0}, E_SHAPE), ({"C": 48}, E_SHAPE), ({"C": 100}, E_SHAPE)]
    tq = [({"Tq": T}, E_SHAPE) for T in T_BAD + (5, 8, 10)]
    fwd = entry(lib.sdf_qk_gate_f32_fwd, "q k e Tq rows C kind tau vth soft vr pw pb st", q=P, k=P, e=P, Tq=2, rows=64, C=96, kind=0,
                tau=2.0, vth=0.1, soft=1, vr=0.0, pw=None, pb=None, st=None)
    run(fwd, each("q k e", None, E_NULL) + each("q k e", ODD16, E_ALIGN) + geo + tq + [
        ({"kind": 3}, E_DTYPE), ({"kind": 1}, E_NULL), ({"kind": 1, "pw": P}, E_NULL), ({"tau": 0.5}, E_SHAPE), ({"tau": 1.0}, E_SHAPE),
        ({"q": None, "e": ODD16}, E_NULL), ({"k": ODD16, "kind": 3}, E_ALIGN), ({"k": ODD16, "rows": 0}, E_ALIGN),
        ({"Tq": 3, "kind": 3}, E_DTYPE), ({"Tq": 3, "rows": 0}, E_SHAPE), ({"kind": 1, "pw": P, "pb": P, "Tq": 3}, E_SHAPE)])

    bwd = entry(lib.sdf_qk_gate_bwd, "q k ge gq gk Tq rows C kind tau vth soft vr det sur alpha pw pb gW gb ws wsb st", q=P, k=P, ge=P,
                gq=P, gk=P, Tq=2, rows=64, C=96, kind=0, tau=2.0, vth=0.1, soft=1, vr=0.0, det=1, sur=0, alpha=2.0, pw=None, pb=None,
                gW=None, gb=None, ws=None, wsb=0, st=None)
    psn = dict(kind=1, pw=P, pb=P, gW=P, gb=P, ws=P, wsb=BIG)
    need = lib.sdf_qk_gate_bwd_workspace_bytes(2, 64, 96)
    assert need == 6 * 6 * 4
    run(bwd, each("q k ge gq gk", None, E_NULL) + each("q k ge gq gk", ODD16, E_ALIGN) + geo + tq + [
        ({"kind": 3}, E_DTYPE), ({"sur": 1}, E_DTYPE), ({"tau": 0.5}, E_SHAPE), ({"tau": 1.0}, E_SHAPE),
        ({"q": None, "sur": 1}, E_NULL), ({"sur": 1, "gq": ODD16}, E_DTYPE), ({"gq": ODD16, "rows": 0}, E_ALIGN),
        ({"gq": ODD16, "Tq": 3}, E_ALIGN), ({"kind": 3, "Tq": 3}, E_DTYPE)] + [
        (dict(psn, **{n: None}), E_NULL) for n in "pw pb gW gb ws".split()] + [
        (dict(psn, wsb=need - 1), E_SHAPE), (dict(psn, ws=ODD4), E_SHAPE), (dict(psn, Tq=3), E_SHAPE), (dict(psn, Tq=0), E_SHAPE),
        (dict(psn, wsb=need - 1, sur=1), E_SHAPE), (dict(psn, sur=1), E_DTYPE), (dict(psn, gk=ODD16), E_ALIGN),
        (dict(psn, wsb=need - 1, q=None), E_NULL)])

    pfwd = entry(lib.sdf_qk_gate_plif_f32_fwd, "q k e pk Tq rows C vth soft vr st", q=P, k=P, e=P, pk=P, Tq=2, rows=64, C=96, vth=0.1,
                 soft=1, vr=0.0, st=None)
    run(pfwd, each("q k e pk", None, E_NULL) + each("q k e", ODD16, E_ALIGN) + geo + tq + [
        ({"pk": ODD4}, E_ALIGN), ({"pk": None, "Tq": 3}, E_NULL), ({"e": ODD16, "rows": 0}, E_ALIGN), ({"e": ODD16, "Tq": 3}, E_ALIGN)])

    pbwd = entry(lib.sdf_qk_gate_plif_bwd, "q k ge gq gk pk gpk ws wsb Tq rows C vth soft vr det sur alpha st", q=P, k=P, ge=P, gq=P,
                 gk=P, pk=P, gpk=P, ws=P, wsb=BIG, Tq=2, rows=64, C=96, vth=0.1, soft=1, vr=0.0, det=1, sur=0, alpha=2.0, st=None)
    need = lib.sdf_qk_gate_plif_bwd_workspace_bytes(2, 64, 96)
    assert need == 6 * 4
    run(pbwd, each("q k ge gq gk pk gpk ws", None, E_NULL) + each("q k ge gq gk", ODD16, E_ALIGN) + each("pk gpk ws", ODD4, E_ALIGN)
        + geo + tq + [
        ({"sur": 1}, E_DTYPE), ({"wsb": need - 1}, E_SHAPE),
        ({"ws": None, "sur": 1}, E_NULL), ({"sur": 1, "Tq": 3}, E_DTYPE), ({"sur": 1, "rows": 0}, E_DTYPE),
        ({"Tq": 3, "gq": ODD16}, E_SHAPE), ({"rows": 0, "gq": ODD16}, E_SHAPE), ({"wsb": need - 1, "gq": ODD16}, E_SHAPE)])


def test_workspace_sizes_follow_the_grid_rule(lib):
    """One row of partials per workgroup: 4 neurons per lane and 256 lanes per workgroup (the PSN backward: 2 per lane at T >= 8,
    and at most 512 workgroups of a grid-stride loop)."""
    quad_blocks = lambda N: (N // 4 + 255) // 256
    for N in (4, 1024, 1028, 4096 * 256 + 4):
        for T in T_STREAM:
            assert lib.sdf_plif_bwd_workspace_bytes(T, N) == quad_blocks(N) * 4, (T, N)
            psn_blocks = min((N // (2 if T >= 8 else 4) + 255) // 256, 512)
            assert lib.sdf_psn_bwd_workspace_bytes(T, N) == (psn_blocks * (T * T + T) * 4 if T <= 10 else 0), (T, N)
        for T in T_GLIF:
            assert lib.sdf_glif_bwd_workspace_bytes(T, N) == quad_blocks(N) * (5 + T) * 4, (T, N)
    for T in (0, 3, 7, 12):
        assert lib.sdf_glif_bwd_workspace_bytes(T, 4096) == 0 and lib.sdf_plif_bwd_workspace_bytes(T, 0) == 0
    assert lib.sdf_plif_bwd_workspace_bytes(0, 4096) == 0 and lib.sdf_psn_bwd_workspace_bytes(0, 4096) == 0
    assert lib.sdf_psn_bwd_workspace_bytes(10, 0) == 0
    for Tq in T_GATE:
        for rows, Cc in ((1, 32), (9, 96), (64, 96), (11, 192)):
            blocks = (rows * (Cc // 32) * 8 + 255) // 256
            assert lib.sdf_qk_gate_bwd_workspace_bytes(Tq, rows, Cc) == blocks * (Tq * Tq + Tq) * 4
            assert lib.sdf_qk_gate_plif_bwd_workspace_bytes(Tq, rows, Cc) == blocks * 4
