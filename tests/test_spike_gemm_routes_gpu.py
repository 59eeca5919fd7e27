"""sdf_spike_gemm_fwd on 16-bit weight planes (nsplit 1, 2, 3) on every route its dispatcher can take (csrc/spike_gemm.hip), against
float64 references (tests/spike_gemm_cases.py).

Three kernels sit behind the entry point: the streaming kernel spike_gemm_kernel<NSPLIT, NB, RB, TT, WAVES, false> in four tile
configurations, the ping-pong kernel spike_mm_pp_kernel<NSPLIT, TT, false>, and splitk_reduce_kernel behind the ping-pong kernel's
split-K plan.  Every case

  * names its route LITERALLY in its table - kernel, template arguments, workgroups, whether a reduce pass follows - and asserts
    through hip.launch_log() that exactly those launches happened, in that order, with 64 * WAVES / 768 / 256 threads;
  * writes into a slice of a larger buffer: 64 guard rows on each side (guard columns too with ldo > N), NaN (fp32) or the byte 7
    (spikes) everywhere beforehand; afterwards everything that is not a result holds the same bits - the guards, the rows a row map
    does not name and the rows it drops - and no NaN / 7 is left where a result belongs;
  * runs the call twice: bit-equal.

References.  EXACT cases (weights s * 2^e * (1 + 2^-9 + 2^-17), at most 16 ones per row of A): torch.equal with the float64 product,
which is the fp32 result in any accumulation order (the premise is asserted on the CPU below); a dropped or mis-scaled plane, a wrong
accumulator scale or a K chunk added twice fails them outright.  RANDOM cases: per element |got - ref64| <= GAMMA * mag, mag =
|alpha| (A |W|^T + |bias|) + |beta| + |resid|, and exactly 0 where mag is 0.  FUSED-NEURON cases: O.delta_consistent on the float64
pre-activation cast to fp32, delta = 16 * 2^-23 * max(rms, v_th): 0 unexplained decisions, spike rate in (0.03, 0.97), at most 1e-4
of the decisions ambiguous; and exact-operand cases whose threshold is the weights' significand, where dozens to thousands of first-step decisions sit ON
the threshold and the spikes must equal the reference neuron's.

In the (b, t, hw) addressing the position count 2 HW is even and a tile's positions are too, so "one more than a multiple of a
tile's positions" is run in the time-major addressing and "two more" in that one.

Measured on an MI355X (all random cases of this file), largest |err| / mag per kernel and weight format (1 / 2 / 3 planes):
  spike_gemm_kernel      8.3e-8 / 2.3e-7 / 2.8e-7    -> GAMMA 2^-19 (1.9e-6): the smallest power of two >= 4 x 2.8e-7
  spike_mm_pp_kernel     6.9e-8 / 2.3e-7 / 2.1e-7    -> GAMMA 2^-20 (9.5e-7)
  splitk_reduce_kernel   6.4e-8 / 9.6e-8 / 1.1e-7    -> GAMMA 2^-21 (4.8e-7)
(the factor 4 covers other accumulation orders when a tile shape changes; all far below the project's 1e-5 for these products).
Fused neuron: 5.1 M decisions in the random cases, 19 of them ambiguous, 0 differ from the reference's, 0 unexplained.
Run time there: the 530 GPU cases in 6.3 s together; the slowest (the persistent 512 x 96 configuration, a 50 MB output compared
element by element on the host) 0.54 s, every case outside the persistent table below 0.25 s.
"""
import functools

import pytest
import torch

import spike_gemm_cases as G
from sdformerflow_amd import hip

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD = G.GUARD
STREAM, PP, REDUCE = "spike_gemm_kernel", "spike_mm_pp_kernel", "splitk_reduce_kernel"
GAMMA = {STREAM: 2.0 ** -19, PP: 2.0 ** -20, REDUCE: 2.0 ** -21}      # from the measured figures above; none may exceed 1e-5
NS = (1, 2, 3)
SWITCHES = ("SDF_GEMM_CFG", "SDF_GEMM_WS", "SDF_GEMM_WGS", "SDF_KSPLIT_MULT", "SDF_PP_PAIR")

# the four configurations of the streaming kernel: (NB, RB, WAVES) - a tile is 32 RB WAVES rows x 32 NB columns
CFG = {0: (3, 2, 8), 1: (3, 1, 8), 2: (1, 2, 4), 3: (1, 1, 4)}


def stream(ns, cfg, tt, wgs):
    nb, rb, waves = CFG[cfg]
    return (STREAM, (ns, nb, rb, tt, waves), 64 * waves, wgs)


def pp(ns, tt, wgs):
    return (PP, (ns, tt), 768, wgs)


def reduce(wgs):
    return (REDUCE, None, 256, wgs)


def _assert_launches(log, want):
    """Exactly the launches `want`, in order: (kernel, template arguments, threads, workgroups) each; the demangled or the mangled name."""
    assert len(log.rows) == len(want), (log.rows, want)
    for (name, wgs, threads, _, _), (kernel, targs, wthreads, wwgs) in zip(log.rows, want):
        if targs is None:
            names = (kernel, kernel)
        else:
            names = (f"{kernel}<{', '.join(str(a) for a in targs)}, false>", f"{kernel}I{''.join(f'Li{a}E' for a in targs)}Lb0EE")
        assert names[0] in name or names[1] in name, (name, names)
        assert (threads, wgs) == (wthreads, wwgs), (name, threads, wgs, wthreads, wwgs)


def _route(monkeypatch, cfg=None, ws=None, wgs=None):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for name, v in (("SDF_GEMM_CFG", cfg), ("SDF_GEMM_WS", ws), ("SDF_GEMM_WGS", wgs)):
        if v is not None:
            monkeypatch.setenv(name, str(v))


@functools.lru_cache(maxsize=None)
def _planes(N, K, ns, exact):
    return hip.split_weight(G.weights(N, K, ns == 1, exact).to(DEV), ns)


# ---------------------------------------------------------------------------------------------------- fp32 epilogue
def _run_f32(c, lay, ns, exact):
    M, N, K, f, ld, c0, rows = c["M"], c["N"], c["K"], c["flags"], lay["ld"], lay["c0"], c["rows"]
    buf = lay["init"].to(DEV)
    inside = slice(GUARD * ld + c0, (GUARD + rows) * ld)
    out = buf.view(-1)[inside]
    resid = out if "res_in" in f else None
    if "res_sep" in f:
        rbuf = lay["resid"].to(DEV)
        resid = rbuf.view(-1)[inside]
    abuf, a0, lda = G.a_layout(c)
    abuf = abuf.to(DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    rowmap = c["dst"].to(torch.int32).to(DEV) if "map" in f else None
    Wp = _planes(N, K, ns, exact)
    with hip.launch_log() as log:
        hip.spike_gemm(abuf.view(-1)[a0:], Wp, out, M, N, K, lda=lda, ldo=ld, bias=dev(c["bias"]), alpha=dev(c["alpha"]), beta=dev(c["beta"]),
                       resid=resid, out_rowmap=rowmap, zg=c["zg"])
    torch.cuda.synchronize()
    return buf.cpu(), log


def _check_f32(monkeypatch, env, want, M, N, K, ns, exact, feat="plain", zg=None, bound=None):
    _route(monkeypatch, **env)
    c = G.f32_case(M, N, K, ns == 1, exact, feat, zg)
    lay = G.f32_layout(c)
    got, log = _run_f32(c, lay, ns, exact)
    _assert_launches(log, want)
    w = lay["written"]
    assert torch.equal(got.view(torch.int32)[~w], lay["init"].view(torch.int32)[~w]), "a store outside the rows and columns of the result"
    res, ref = got[w], lay["ref"][w]
    assert not torch.isnan(res).any(), "an element of the result was never written"
    if exact:
        assert torch.equal(res, ref.float()), f"{int((res != ref.float()).sum())} of {res.numel()} elements differ from the exact product"
    else:
        mag = lay["mag"][w]
        zero = mag == 0
        assert bool((res[zero] == 0).all()), "an element without any term is not exactly 0"
        if zg is None and M > 2 and feat == "plain":
            assert bool(zero.any())                                         # (the silent row)
        ratio = ((res.double() - ref).abs()[~zero] / mag[~zero]).max().item()
        kernel = bound or want[-1][0]
        print(f"\nSGEMM f32 {kernel} ns{ns} {M}x{N}x{K} {feat} err/mag {ratio:.3e}")
        assert ratio <= GAMMA[kernel], ratio
    again, _ = _run_f32(c, lay, ns, exact)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two calls differ"


FEATS = ("bias", "bn", "res_in", "res_sep", "map", "ldo", "lda", "all")
ZGS = ((3, 2, 4, 5), (6, 2, 4, 5), (3, 2, 8, 5, 4))                       # (nH, Tq, B_, N1[, windows per replica]): M = Tq B_ N1, K = 32 nH

# streaming kernel, fp32 epilogue (SDF_GEMM_WS=0, SDF_GEMM_CFG=cfg): (cfg, M, N, K, workgroups = tiles)
#   M = 1 | M = tile rows + 1 on two column blocks, K = one full stage of 96 + a partial one | K = 32 and K = 128
STREAM_F32 = [(0, 1, 96, 32, 1), (0, 513, 192, 160, 4), (0, 77, 96, 128, 1),
              (1, 1, 96, 32, 1), (1, 257, 192, 160, 4), (1, 77, 96, 128, 1),
              (2, 1, 32, 32, 1), (2, 257, 64, 160, 4), (2, 77, 32, 128, 1),
              (3, 1, 32, 32, 1), (3, 129, 64, 160, 4), (3, 77, 32, 128, 1)]
# the epilogue features run on the second shape of each configuration
STREAM_FEAT = [(0, 513, 192, 160, 4), (1, 257, 192, 160, 4), (2, 257, 64, 160, 4), (3, 129, 64, 160, 4)]
# head scramble: (cfg, N); one tile
STREAM_ZG = [(0, 96), (1, 96), (2, 32), (3, 32)]
# persistent: SDF_GEMM_WGS=1 -> 256 workgroups on 86 row tiles x 3 column blocks = 258 tiles: workgroups 0 and 1 walk two tiles each
STREAM_PERSIST = [(0, 43521, 288, 32), (1, 21761, 288, 32), (2, 21761, 96, 32), (3, 11008, 96, 32)]


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("cfg,M,N,K,wgs", STREAM_F32)
def test_stream_f32(monkeypatch, cfg, M, N, K, wgs, ns, exact):
    _check_f32(monkeypatch, dict(cfg=cfg, ws=0), [stream(ns, cfg, 0, wgs)], M, N, K, ns, exact)


@gpu
@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("cfg,M,N,K,wgs", STREAM_FEAT)
def test_stream_f32_epilogue(monkeypatch, cfg, M, N, K, wgs, ns, feat):
    _check_f32(monkeypatch, dict(cfg=cfg, ws=0), [stream(ns, cfg, 0, wgs)], M, N, K, ns, False, feat)


@gpu
@pytest.mark.parametrize("zg", ZGS, ids=lambda z: "zg" + "-".join(map(str, z)))
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("cfg,N", STREAM_ZG)
def test_stream_f32_head_scramble(monkeypatch, cfg, N, ns, zg):
    _check_f32(monkeypatch, dict(cfg=cfg, ws=0), [stream(ns, cfg, 0, 1)], zg[1] * zg[2] * zg[3], N, 32 * zg[0], ns, False, zg=zg)


@gpu
@pytest.mark.parametrize("ns,exact", [(1, False), (2, False), (3, False), (3, True)])
@pytest.mark.parametrize("cfg,M,N,K", STREAM_PERSIST)
def test_stream_f32_persistent(monkeypatch, cfg, M, N, K, ns, exact):
    _check_f32(monkeypatch, dict(cfg=cfg, ws=0, wgs=1), [stream(ns, cfg, 0, 256)], M, N, K, ns, exact)


# ping-pong kernel, fp32 epilogue, no split-K (SDF_GEMM_WS=2; K < 256): (M, N, K, workgroups).  256 x 96 tiles, stages of 64
PP_F32 = [(1, 96, 64, 1), (1, 96, 96, 1), (1, 96, 160, 1), (1, 288, 64, 3), (1, 288, 96, 3), (1, 288, 160, 3),
          (257, 96, 64, 2), (257, 96, 96, 2), (257, 96, 160, 2), (257, 288, 64, 6), (257, 288, 96, 6), (257, 288, 160, 6),
          (4097, 96, 96, 9),              # 17 items on 9 workgroups: one of them has a single item
          (1281, 288, 96, 9)]             # 18 items on 9 workgroups: two each


@gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("ns", NS)
@pytest.mark.parametrize("M,N,K,wgs", PP_F32)
def test_pp_f32(monkeypatch, M, N, K, wgs, ns, exact):
    _check_f32(monkeypatch, dict(ws=2), [pp(ns, 0, wgs)], M, N, K, ns, exact)


@gpu
@pytest.mark.parametrize("feat", FEATS)
@pytest.mark.parametrize("ns", NS)
def test_pp_f32_epilogue(monkeypatch, ns, feat):
    _check_f32(monkeypatch, dict(ws=2), [pp(ns, 0, 6)], 257, 288, 160, ns, False, feat)


@gpu
@pytest.mark.parametrize("zg", ZGS, ids=lambda z: "zg" + "-".join(map(str, z)))
@pytest.mark.parametrize("ns", NS)
def test_pp_f32_head_scramble(monkeypatch, ns, zg):
    _check_f32(monkeypatch, dict(ws=2), [pp(ns, 0, 1)], zg[1] * zg[2] * zg[3], 96, 32 * zg[0], ns, False, zg=zg)


@gpu
@pytest.mark.parametrize("feat,exact", [("plain", True), ("plain", False), ("sk_all", False)])
@pytest.mark.parametrize("ns", NS)
def test_pp_f32_splitk(monkeypatch, ns, feat, exact):
    """M = 300, N = 96, K = 320: 2 tiles, 5 stages split 3 + 2 over 2 chunks = 4 items; the reduce pass has 300 * 24 quads on 29
    workgroups and carries the whole epilogue."""
    _check_f32(monkeypatch, dict(ws=2), [pp(ns, 0, 4), reduce(29)], 300, 96, 320, ns, exact, feat)


# ---------------------------------------------------------------------------------------------------- fused neuron
def _run_sn(c, ns, exact):
    T, pos, N, K = c["T"], c["pos"], c["N"], c["K"]
    rows = T * pos
    buf = torch.full((GUARD + rows + GUARD, N), 7, dtype=torch.uint8, device=DEV)
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    p = hip.NeuronParams(c["neuron"], G.TAU, c["v_th"], c["v_reset"], dev(c["psn_w"]), dev(c["psn_b"]))
    A, Wp = c["A"].to(DEV), _planes(N, K, ns, exact)
    with hip.launch_log() as log:
        hip.spike_gemm_sn(A, Wp, buf[GUARD:GUARD + rows], N, K, T, *G.sn_addressing(T, pos, c["layout"]), p, alpha=dev(c["alpha"]),
                          beta=dev(c["beta"]), add=dev(c["add"]), add_prows=7 if c["add"] is not None else 0)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:GUARD] == 7).all()) and bool((got[GUARD + rows:] == 7).all()), "a store outside `out_spike`"
    got = got[GUARD:GUARD + rows]
    assert bool((got <= 1).all()), "a spike row was never written"
    return got, log


def _check_sn(monkeypatch, env, want, T, pos, N, K, ns, kind, layout, exact=False):
    _route(monkeypatch, **env)
    c = (G.sn_exact_case if exact else G.sn_case)(T, pos, N, K, ns == 1, kind, layout)
    got, log = _run_sn(c, ns, exact)
    _assert_launches(log, want)
    s = G.sn_rows(got, T, pos, layout)
    if exact:
        ref = G.sn_reference(c)
        assert torch.equal(s.float(), ref), f"{int((s.float() != ref).sum())} of {ref.numel()} spikes differ on exact operands"
    else:
        rep = G.sn_report(c, s)
        print(f"\nSGEMM sn {want[0][0]} ns{ns} T{T} {kind} {layout} {rep}")
        assert rep["unexplained"] == 0, rep
        assert rep["ambiguous"] <= 1e-4 * rep["n"], rep
        assert 0.03 < s.float().mean().item() < 0.97
    again, _ = _run_sn(c, ns, exact)
    assert torch.equal(got, again), "two calls differ"


# streaming kernel, fused neuron (SDF_GEMM_WS=0, SDF_GEMM_CFG=cfg): every legal (cfg, T) with P = the positions of one tile
# = 2 WAVES (16 RB / T); N = two column blocks; 2 row tiles x 2 column blocks = 4 workgroups everywhere
SN_STREAM = [(0, 2, 256), (0, 4, 128), (0, 5, 96), (0, 10, 48), (0, 20, 16),
             (1, 2, 128), (1, 4, 64), (1, 5, 48), (1, 10, 16),
             (2, 2, 128), (2, 4, 64), (2, 5, 48), (2, 10, 24), (2, 20, 8),
             (3, 2, 64), (3, 4, 32), (3, 5, 24), (3, 10, 8)]
SN_STREAM_N = {0: 192, 1: 192, 2: 64, 3: 64}
SN_K = 160                                      # the streaming kernel: 96 + 64; the ping-pong kernel: 64 + 64 + 32
# one pair per T for IF, LIF with v_reset = 0, the one-plane format and the further exact cases
SN_STREAM_ONE = [(3, 2, 64), (2, 4, 64), (1, 5, 48), (0, 10, 48), (2, 20, 8)]


def _sn_stream_cases():
    out = []
    for cfg, T, P in SN_STREAM:
        for ns in (2, 3):
            out += [(cfg, T, P + 1, ns, "lif", "tm", False), (cfg, T, P + 2, ns, "psn", "bt", False)]
        out += [(cfg, T, P + 1, 3, "lif", "tm", True)]
    for cfg, T, P in SN_STREAM_ONE:
        out += [(cfg, T, P + 2, 3, "if", "bt", False), (cfg, T, P + 1, 2, "lif0", "tm", False), (cfg, T, P + 1, 1, "lif", "tm", False),
                (cfg, T, P + 2, 2, "psn", "bt", True), (cfg, T, P + 1, 1, "lif", "tm", True), (cfg, T, P + 1, 3, "if", "tm", True)]
    return out


def _sn_id(v):
    return {True: "exact", False: "random"}.get(v, str(v)) if isinstance(v, bool) else None


@gpu
@pytest.mark.parametrize("cfg,T,pos,ns,kind,layout,exact", _sn_stream_cases(), ids=_sn_id)
def test_stream_fused_neuron(monkeypatch, cfg, T, pos, ns, kind, layout, exact):
    _check_sn(monkeypatch, dict(cfg=cfg, ws=0), [stream(ns, cfg, T, 4)], T, pos, SN_STREAM_N[cfg], SN_K, ns, kind, layout, exact)


# ping-pong kernel, fused neuron (SDF_GEMM_WS=2): (T, P = 8 (32 / T), formats); 2 row tiles x N / 96 column blocks
SN_PP = [(2, 128, (1, 2, 3)), (10, 24, (1, 2, 3)), (20, 8, (2,))]


def _sn_pp_cases():
    out = []
    for T, P, formats in SN_PP:
        for N, wgs in ((96, 2), (288, 6)):
            for ns in formats:
                out += [(T, P + 1, N, wgs, ns, "lif", "tm", False), (T, P + 2, N, wgs, ns, "psn", "bt", False), (T, P + 1, N, wgs, ns, "lif", "tm", True)]
        out += [(T, P + 2, 96, 2, 2, "if", "bt", False), (T, P + 1, 96, 2, 2, "lif0", "tm", False), (T, P + 2, 96, 2, 2, "psn", "bt", True),
                (T, P + 1, 96, 2, 2, "if", "tm", True)]
    return out


@gpu
@pytest.mark.parametrize("T,pos,N,wgs,ns,kind,layout,exact", _sn_pp_cases(), ids=_sn_id)
def test_pp_fused_neuron(monkeypatch, T, pos, N, wgs, ns, kind, layout, exact):
    _check_sn(monkeypatch, dict(ws=2), [pp(ns, T, wgs)], T, pos, N, SN_K, ns, kind, layout, exact)


# ---------------------------------------------------------------------------------------------------- what the dispatcher does today
@gpu
def test_default_f32_takes_cfg3(monkeypatch):
    _check_f32(monkeypatch, {}, [stream(3, 3, 0, 9)], 300, 96, 96, 3, False)                    # 3 row tiles x 3 column blocks


@gpu
def test_default_splitk_takes_pingpong(monkeypatch):
    """M = 64, N = 96, K = 2048: one tile, 32 stages in 16 chunks = 16 items on 8 workgroups; 64 * 24 quads on 6."""
    _check_f32(monkeypatch, {}, [pp(3, 0, 8), reduce(6)], 64, 96, 2048, 3, False)


# (T, positions, N, format, expected launch).  The last two ask for a configuration that is illegal there: the switch is ignored
DEFAULT_SN = [(2, 65, 96, 3, {}, stream(3, 3, 2, 6)),           # cfg 3: 2 row tiles of 64 positions x 3 column blocks
              (5, 49, 96, 3, {}, stream(3, 1, 5, 2)),           # cfg 1: 2 x 1
              (10, 25, 64, 3, {}, stream(3, 2, 10, 4)),         # N is no multiple of 96 -> cfg 2: 2 x 2
              (10, 25, 96, 3, {}, pp(3, 10, 2)),
              (20, 9, 96, 3, {}, stream(3, 2, 20, 6)),          # three planes: no ping-pong form of T = 20 -> cfg 2: 2 x 3
              (20, 9, 96, 2, {}, pp(2, 20, 2)),
              (20, 9, 96, 3, dict(cfg=1, ws=0), stream(3, 2, 20, 6)),      # T = 20 does not fit one row block: SDF_GEMM_CFG=1 is ignored
              (5, 49, 64, 3, dict(cfg=0), stream(3, 2, 5, 4))]             # 96-wide tiles need N % 96 == 0: SDF_GEMM_CFG=0 is ignored


@gpu
@pytest.mark.parametrize("T,pos,N,ns,env,want", DEFAULT_SN, ids=[f"T{r[0]}-N{r[2]}-ns{r[3]}-" + ("".join(f"{k}{v}" for k, v in r[4].items()) or "default") for r in DEFAULT_SN])
def test_default_fused_neuron_routes(monkeypatch, T, pos, N, ns, env, want):
    _check_sn(monkeypatch, env, [want], T, pos, N, 96, ns, "lif", "tm")


# ---------------------------------------------------------------------------------------------------- the premises, on the CPU
def _f32_exact_shapes():
    shapes = {(M, N, K) for _, M, N, K, _ in STREAM_F32} | {(M, N, K) for M, N, K, _ in PP_F32} | {(300, 96, 320)}
    return sorted(shapes | {(M, N, K) for _, M, N, K in STREAM_PERSIST})


@pytest.mark.parametrize("one_plane", [False, True])
def test_exact_products_are_representable(one_plane):
    """The premise of the exact cases: the float64 product is an fp32 number, and so is every partial sum (the sum of the absolute
    terms is one too, below 2^5, on a grid of 2^-19)."""
    for M, N, K in _f32_exact_shapes():
        c = G.f32_case(M, N, K, one_plane, True)
        for v in (c["y"], c["mag"]):
            assert torch.equal(v.float().double(), v)
        assert c["mag"].max().item() < 32 and torch.equal(c["mag"] * 2 ** 19, (c["mag"] * 2 ** 19).round())
        assert int(c["A"].sum(1).max()) <= 16
    W = G.weights(96, 96, one_plane, True)
    bits = W.view(torch.int32)
    assert int((bits & 0xFFFF).ne(0).sum()) == (0 if one_plane else W.numel())           # more than one bf16 plane is needed
    assert float(W.abs().max()) >= 1.0


def test_exact_neuron_cases_sit_on_the_threshold():
    for case in [c for c in _sn_stream_cases() if c[-1]]:
        cfg, T, pos, ns, kind, layout, _ = case
        c = G.sn_exact_case(T, pos, SN_STREAM_N[cfg], SN_K, ns == 1, kind, layout)
        assert torch.equal(c["x"].double(), c["x64"])
        assert G.on_threshold(c) >= 8, (case, G.on_threshold(c))
        assert 0.03 < G.sn_reference(c).mean().item() < 0.97, case
    for case in [c for c in _sn_pp_cases() if c[-1]]:
        T, pos, N, _, ns, kind, layout, _ = case
        c = G.sn_exact_case(T, pos, N, SN_K, ns == 1, kind, layout)
        assert torch.equal(c["x"].double(), c["x64"])
        assert G.on_threshold(c) >= 8, (case, G.on_threshold(c))
        assert 0.03 < G.sn_reference(c).mean().item() < 0.97, case


def test_random_neuron_cases_are_not_on_the_threshold():
    """The reference's own spikes: at most 1e-4 of a case's decisions are within delta of the threshold, the rate is inside (0.03, 0.97)."""
    cases = [(T, pos, SN_STREAM_N[cfg], SN_K, ns == 1, kind, layout) for cfg, T, pos, ns, kind, layout, ex in _sn_stream_cases() if not ex]
    cases += [(T, pos, N, SN_K, ns == 1, kind, layout) for T, pos, N, _, ns, kind, layout, ex in _sn_pp_cases() if not ex]
    cases += [(T, pos, N, 96, ns == 1, "lif", "tm") for T, pos, N, ns, _, _ in DEFAULT_SN]
    for key in sorted(set(cases)):
        c = G.sn_case(*key)
        ref = G.sn_reference(c)
        rep = G.sn_report(c, ref)
        assert rep["unexplained"] == 0 and rep["flips"] == 0, (key, rep)
        assert rep["ambiguous"] <= 1e-4 * rep["n"], (key, rep)
        assert 0.03 < ref.mean().item() < 0.97, key
