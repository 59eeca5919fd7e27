"""Parity of the int8 digit-plane kernels of the spiking Swin block, instantiation by instantiation: res_pm_kernel / res_front_kernel
(csrc/ms_res.hip), wide_pm_kernel / wide_front_kernel (csrc/ms_wide.hip) and smallm_kernel as fc2 (csrc/ms_smallm.hip), through
hip.qk_attn, hip.ms_mlp, hip.ms_patch_merge and the row-loop forms of hip.spike_gemm / hip.spike_deconv3x3s2.  Inputs, float64
references, checks and the DERIVED launch lines are tests/digit_cases.py's (plain CPU code); tests/test_ms_wide_gpu.py keeps the
workload's own shapes, tests/test_digit_routes_gpu.py the recorded launch lists.

Every GPU case (test_case[name], name in digit_cases.CASES)
  route    the launches of the call, read through hip.launch_log(), equal the lines digit_cases.route derives from the dispatch code;
  repeat   the call runs twice into fresh buffers: the same launches, every output bit-equal;
  guards   x is a slice of a NaN buffer with 64 guard rows on each side; the emit buffers and BOTH workspaces (hip.ms_mlp's `ws`, hip.qk_attn's
           `ws`) are 256-aligned slices of u8 buffers filled with 7: afterwards the guards and everything past the documented extents
           (sdf_ms_mlp_workspace_bytes, sdf_qk_attn_workspace_bytes, (rows + 80) C of a tiled emission) hold the same bits, no NaN and
           no 7 stands where a result belongs, and without the tape the q | k region keeps its 7s;
  neurons  different settings of one class wherever a call takes several, the emitted neuron of ANOTHER class than the block's;
  steps    MLP: SN1 bit-equal, SN2 delta-consistent on the kernel's own SN1, output within 1e-5 of its range on the kernel's own SN2;
           attention: slice spikes bit-equal, q | k delta-consistent (positional term on k), E == k AND SN2_q(head sums of the kernel's own
           q), the projection through the head scramble and the scatter within 1e-5; the emitted spikes bit-equal to the neuron on the
           kernel's own updated x; fp32 products (merge, plain product, transposed convolution) within 1e-6 of the range;
  forms    the tape form and the production form (no tape, tiled hand-over) give the same x bit for bit; a tiled emission of the
           attention, handed to hip.ms_mlp(s1_ready=True), gives the x of the MLP on its own first neuron bit for bit.  (That is how the
           CONTENT of a tiled emission is checked - a wrong spike changes x; directly, only what lies behind its (x_rows + 80) C extent is.
           The hand-over call itself asserts no route: the MLP's routes are the mlp_* cases'.)
test_families[name]: wherever another kernel family serves the same call (row loop <-> K ring from 192 channels on in steps of 64, the
merge with the row loop switched off, fc2 on the small-M kernel <-> the K ring at C = 384 and <-> the row loop at C = 192) every output is
bit-equal between the two.

Which test covers which instantiation (test_the_cases_reach_every_instantiation asserts the union equals the enumeration, by name)
  res_pm_kernel<T, 1, n, 0, sk, false>      fc1: mlp_res64 / res96 / res160 / res192 (small-K), mlp_res320 / res384 (not)
  res_pm_kernel<T, 3, n, 0, sk, false>      fc2 + emit: mlp_res64_*_emit (K = 256), mlp_res192_*_emit (K = 768), mlp_res320 (K = 960); the projection + emit:
                                            attn_res64 / 96 / 160 / 192 (small-K), attn_res384 / res512 (not)
  res_pm_kernel<T, 2, 0, 0, sk, strip>      fc2 on tiled (strip off) / row-major (tape: strip on) hidden spikes, the projection, gemm_k* (strip on;
                                            *_nostrip: SDF_RES_STRIP=0)
  res_pm_kernel<T, 2, 0, 2, sk, strip>      merge_res64 (small-K) / res96 / res160 / res256, *_nostrip
  res_pm_kernel<T, 2, 0, 3, sk, strip>      deconv64 (small-K) / deconv96, *_nostrip
  res_front_kernel<n, keep>                 attn_res* (keep = the tape)
  wide_pm_kernel<T, 2 | 3, 1, n>            fc1: mlp_wide384_* (three blocks: *_cb3, *_passes2, *_above1024), mlp_wide320
  wide_pm_kernel<T, 2, 2 | 3, n>            fc2 of mlp_wide* and of mlp_res384 with the small-M kernel off; the projection of attn_wide*
  wide_pm_kernel<T, 2, 2, 0, 2>             merge_wide320
  wide_front_kernel<2 | 4, n, keep>         attn_wide* (4: *_rb4_*)
  smallm_kernel<T, 2 | 3, n, 0, true, 2>    mlp_res384_*_smallm* (N = 384, K = 1 536), mlp_res192_*_smallm* (N = 192, K = 768: surplus workgroups)
  both families, C = 192 .. 768 by 64       attn_fam* / mlp_fam* (and every default-route case of such a C) in test_families

Measured on an MI355X (recorded - the file prints them as "DIGPAR ..." lines; no bound is set from these numbers, the bounds are the
project's own, see digit_cases.py).  Decisions of the checked neurons, summed over the cases of a kernel:
  res_pm_kernel     fc1 + SN2    52 cases   32 647 680 decisions   143 ambiguous   0 flipped
  wide_pm_kernel    fc1 + SN2    17 cases   43 635 840 decisions   153 ambiguous   0 flipped
  res_front_kernel  q | k        28 cases   23 077 120 decisions    61 ambiguous   0 flipped
  wide_front_kernel q | k        22 cases   36 284 160 decisions   159 ambiguous   1 flipped      (0 unexplained everywhere)
Largest fp32 error against the range: fc2 res_pm_kernel 1.1e-7, wide_pm_kernel 1.1e-7, smallm_kernel 1.0e-7; the projection res_pm_kernel
1.2e-7, wide_pm_kernel 1.3e-7 (bound 1e-5); merge res_pm_kernel 7.3e-8, wide_pm_kernel 6.7e-8, plain product 9.3e-8, transposed convolution
8.4e-8 (bound 1e-6).  The 145 cases take 7.1 s in all, the slowest (mlp_wide384_T20_above1024) 0.8 s; the file's 216 GPU tests 12.7 s.

The slice map names every row of x exactly once (test_each_shape_sits_where_its_comment_says); its entries of -1 are the padding slots of
the windows: they read as zeros and have no row to write to - a store through one of them lands in a guard row or fails the output check.

Left out on purpose.  K = 272 (K % 16 == 0, not % 32) is a K the row loop's own predicate admits (res_pm_takes) and no entry point passes on:
sdf_spike_gemm_fwd asks K % 32 == 0 of every product, the merge has K = 4 C with C % 32 == 0, the transposed convolution K = 4 Cin with
Cin % 16 == 0.  gemm_k288 is the first build beyond small-K that can be reached; test_k272_is_refused holds the entry point to its refusal.
K = 1 024, the largest resident image, is reached by the merge at C = 256 and the plain product: the MLP at C = 256 (Ch = 1 024, no
multiple of 96) is not served by these kernels (ms_wide_mlp_supports).
"""
import functools
import time

import pytest
import torch

import digit_cases as DC
import stage0_cases as S
import spike_conv_cases as SC
import test_digit_routes_gpu as PINS
from routes_common import logged
from sdformerflow_amd import hip

gpu = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = PINS.SWITCHES
PAD = 4096                                                   # guard bytes on each side of a u8 buffer (a multiple of 256: the slice stays aligned)


def _route(monkeypatch, env):
    """the shipped dispatch, but for the switches a case names"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _np(n):
    """a case's neuron for the library (one object per setting: the PSN tables keep their addresses)"""
    if n.psn_w is None:
        return hip.NeuronParams(n.kind, n.tau, n.v_th, n.v_reset)
    return hip.NeuronParams(n.kind, n.tau, n.v_th, n.v_reset, n.psn_w.to(DEV), n.psn_b.to(DEV))


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _weff(dg):
    """the float64 value of the weight the device's int8 digit planes carry (`_weff` of test_ms_wide_gpu.py)"""
    d = dg.cpu().double()
    return (d[2] * 65536 + d[1] * 256 + d[0]) * dg.sdf_col_scale.cpu().double().view(-1, 1)


class _L:
    """a layer for the library: the two 16-bit planes every entry point asks for, the digit planes (checked against the CPU restatement the
    references multiply by), optionally the digits in fragment order"""

    def __init__(self, W, alpha, beta, bias=None, held=None, tiled=False):
        self.N, self.K = W.shape
        self.Wp = hip.split_weight(_dev(W), 2)
        self.digits = hip.split_weight_i8x3(_dev(W))
        if held is not None:
            assert torch.equal(_weff(self.digits), held), "the device's digit planes differ from their CPU restatement"
        if tiled:
            self.digits_tiled = hip.tile_weight_i8x3(self.digits)
        self.alpha, self.beta, self.bias = _dev(alpha), _dev(beta), _dev(bias)


def _lin(lin, held=None, tiled=False):
    return _L(lin["W"], lin["alpha"], lin["beta"], lin.get("bias"), lin.get("held", held), tiled)


# ---------------------------------------------------------------------------------------------------- guarded buffers
def _f32_guarded(rows, cols, fill=None):
    """(buffer (rows + 2 x 64, cols) of NaN, its middle): x with `fill` copied in, or an output left NaN"""
    buf = torch.full((rows + 2 * DC.GUARD, cols), float("nan"), dtype=torch.float32, device=DEV)
    mid = buf[DC.GUARD:DC.GUARD + rows]
    if fill is not None:
        mid.copy_(fill.reshape(rows, cols))
    return buf, mid


def _f32_guards_hold(buf, rows, what):
    b = buf.view(torch.int32)
    nan = torch.full((1,), float("nan")).view(torch.int32).item()
    assert bool((b[:DC.GUARD] == nan).all()) and bool((b[DC.GUARD + rows:] == nan).all()), f"{what}: a guard row was written"
    assert not torch.isnan(buf[DC.GUARD:DC.GUARD + rows]).any(), f"{what}: NaN left where a result belongs"


def _u8_guarded(nbytes):
    buf = torch.full((nbytes + 2 * PAD,), 7, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[PAD:PAD + nbytes]


def _sevens(t, what):
    assert bool((t == 7).all()), f"{what}: {int((t != 7).sum())} of {t.numel()} bytes were written"


def _spikes(t, what):
    assert int(t.max()) <= 1, f"{what}: a byte that is no spike (7 = never written) stands where a result belongs"
    return t


def _same(a, b, what):
    for k in a:
        if a[k] is not None:
            u, v = a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)
            assert torch.equal(u, v), f"{what}: output `{k}` differs in {int((u != v).sum())} of {u.numel()} bytes"


def _twice(run, want):
    """the call run twice into fresh buffers: the derived launches both times, bit-equal outputs -> the first run's outputs"""
    outs = []
    for _ in range(2):
        got, out = run()
        assert got == want, (got, want)
        outs.append(out)
    _same(outs[0], outs[1], "two calls")
    return outs[0]


# ==================================================================================================== MLP
def _mlp_layers(c, tiled):
    return _lin(c["fc1"]), _lin(c["fc2"], tiled=tiled)


def _mlp_run(c, s, layers, tape, env=None):
    """one hip.ms_mlp of case `s` in the tape or the production form -> (launch lines, outputs on the CPU: the guarded x buffer, the guarded
    workspace buffer, the guarded emit buffer or None)"""
    ntok, C, Ch, D = c["ntok"], c["C"], c["Ch"], c["D"]
    fc1, fc2 = layers
    xb, xm = _f32_guarded(ntok, C, _dev(c["x"]))
    nbytes = DC.mlp_ws_bytes(ntok, C, Ch)
    assert nbytes == hip.lib().sdf_ms_mlp_workspace_bytes(ntok, C, Ch)
    wb, ws = _u8_guarded(nbytes)
    kw = {}
    eb = None
    if s["emit"] is not None:
        eb, ev = _u8_guarded(ntok * C)
        kw["emit_next"] = (ev, _np(DC.emit_neuron(s["emit"], D, s["i"])))
    if tape:
        kw["keep_ws"] = []
    x5 = xm.view(c["B"], D, c["H"], c["W"], C)
    lines, _ = logged(lambda: hip.ms_mlp(x5, fc1, fc2, _np(c["sn1"]), _np(c["sn2"]), ws=ws, **kw))
    return lines, {"x": xb.cpu(), "ws": wb.cpu(), "emit": None if eb is None else eb.cpu()}


def _mlp_checks(c, s, o, tape, name):
    """guards, then the steps of whatever the form left behind -> the updated x (ntok, C)"""
    ntok, C, Ch, D = c["ntok"], c["C"], c["Ch"], c["D"]
    _f32_guards_hold(o["x"], ntok, "x")
    xo = o["x"][DC.GUARD:DC.GUARD + ntok]
    nbytes = DC.mlp_ws_bytes(ntok, C, Ch)
    _sevens(o["ws"][:PAD], "in front of the workspace"), _sevens(o["ws"][PAD + nbytes:], "behind the workspace's documented extent")
    ws = o["ws"][PAD:PAD + nbytes]
    if tape:
        s1 = _spikes(ws[:ntok * C], "SN1's tape").view(ntok, C)
        s2 = _spikes(ws[DC.cdiv(ntok * C, 256) * 256:][:ntok * Ch], "SN2's tape").view(ntok, Ch)
        rep = S.mlp_check(c, s1, s2, xo)
        assert rep["ambiguous"] <= S.AMBIGUOUS_CAP * rep["n"], rep
        err = (xo.double() - DC.mlp_out(c, s2)).abs().max().item() / DC.mlp_out(c, s2).abs().max().item()
        print(f"\nDIGPAR mlp {name} SN2 n {rep['n']} ambiguous {rep['ambiguous']} flips {rep['flips']} x_err/range {err:.2e}")
    if o["emit"] is not None:
        _sevens(o["emit"][:PAD], "in front of the emitted spikes"), _sevens(o["emit"][PAD + ntok * C:], "behind the emitted spikes")
        got = _spikes(o["emit"][PAD:PAD + ntok * C], "the emitted spikes").view(c["B"], D, c["H"] * c["W"], C)
        want = DC.over_time(DC.emit_neuron(s["emit"], D, s["i"]), xo.view(c["B"], D, c["H"] * c["W"], C))
        assert torch.equal(got, want), f"emitted spikes differ from the neuron on the kernel's own x in {int((got != want).sum())} bytes"
        S.check_rate(want)
    return xo


def _mlp_case(monkeypatch, name, env=None):
    s = DC.CASES[name]
    env = s["env"] if env is None else env
    _route(monkeypatch, env)
    c = DC.mlp_case(s["C"], s["Ch"], s["D"], s["B"], s["H"], s["W"], s["cls"], s["i"])
    layers = _mlp_layers(c, s["tiled"])
    o = _twice(lambda: _mlp_run(c, s, layers, s["tape"]), DC.route(s, env))
    xo = _mlp_checks(c, s, o, s["tape"], name)
    # the other form: the same x bit for bit (and the steps, where only the other form keeps the tape)
    other = {**s, "tape": not s["tape"]}
    lines, o2 = _mlp_run(c, other, layers, other["tape"])
    assert lines == DC.route(other, env), (lines, DC.route(other, env))
    xo2 = _mlp_checks(c, other, o2, other["tape"], name)
    assert torch.equal(xo, xo2), "the tape changes the result"
    _same({"emit": o["emit"]}, {"emit": o2["emit"]}, "tape against production form")
    assert not torch.equal(xo, c["x"].reshape(c["ntok"], c["C"]))
    return {"x": o["x"], "emit": o["emit"], "tape": (o if s["tape"] else o2)["ws"][PAD:]}


# ==================================================================================================== attention
def _attn_layers(c):
    lin, held = c["lin"], c["held"]
    p = _lin(lin["p"], held["p"])
    if c["form"] == "stacked":
        wcat = torch.cat([lin["q"]["W"], lin["k"]["W"]], 0)
        dg = hip.split_weight_i8x3(_dev(wcat))
        assert torch.equal(_weff(dg), torch.cat([held["q"], held["k"]], 0))
        kw = dict(qk={"Wp": hip.split_weight(_dev(wcat), 2), "digits": dg, "alpha": _dev(torch.cat([lin["q"]["alpha"], lin["k"]["alpha"]])),
                      "beta": _dev(torch.cat([lin["q"]["beta"], lin["k"]["beta"]])), "add": _dev(torch.cat([torch.zeros_like(c["pe"]), c["pe"]], 1))})
    else:
        kw = dict(q_lin=_lin(lin["q"], held["q"]), k_lin=_lin(lin["k"], held["k"]), pe=_dev(c["pe"]))
    rowmap, B_ = hip.window_slice_map(c["B"], c["D"], c["H"], c["W"], c["window"], c["shift"], DEV)
    assert B_ == c["B_"] and torch.equal(rowmap.cpu(), c["map"])
    zsrc = hip.window_zsrc_map(rowmap, B_, c["Tq"], c["N1"], c["nH"], c["x_rows"])
    return p, kw, rowmap, zsrc


def _attn_run(c, s, layers, tape, keep_dev=False):
    """one hip.qk_attn of case `s` in the tape or the production form -> (launch lines, outputs on the CPU)"""
    p, kw, rowmap, zsrc = layers
    C, D, x_rows = c["Cc"], c["D"], c["x_rows"]
    xb, xm = _f32_guarded(x_rows, C, _dev(c["x"]))
    nbytes, _ = DC.attn_ws_bytes(c)
    assert nbytes == hip.lib().sdf_qk_attn_workspace_bytes(c["B_"], c["Tq"], c["N1"], C)
    wb, ws = _u8_guarded(nbytes)
    kw = dict(kw)
    eb, info = None, {}
    if s["emit"] is not None:
        # the emission lands at the head of an MLP workspace: row-major x_rows C bytes with the tape, else the tiled hand-over layout, (x_rows + 80) C
        eb, ev = _u8_guarded(DC.mlp_ws_bytes(x_rows, C, DC.handover_Ch(C)))
        kw.update(emit=(ev, _np(DC.emit_neuron(s["emit"], D, 0))), info=info)
    if tape:
        kw["keep_ws"] = []
    x5 = xm.view(c["B"], D, c["H"], c["W"], C)
    ns = [_np(n) for n in c["sn"]]
    lines, _ = logged(lambda: hip.qk_attn(x5, rowmap, c["B_"], c["Tq"], c["N1"], c["nH"], p, *ns, x_src=zsrc, ws=ws, **kw))
    assert s["emit"] is None or info.get("emitted") is True, "the wide-stage kernels were not taken"
    out = {"x": xb.cpu(), "ws": wb.cpu(), "emit": None if eb is None else eb.cpu()}
    if keep_dev:
        out["_dev"] = (x5, ev if eb is not None else None)
    return lines, out


def _attn_checks(c, s, o, tape, name):
    C, D, x_rows, M = c["Cc"], c["D"], c["x_rows"], c["Tq"] * c["rows"]
    _f32_guards_hold(o["x"], x_rows, "x")
    xo = o["x"][DC.GUARD:DC.GUARD + x_rows]
    nbytes, (o0, o1, o2) = DC.attn_ws_bytes(c)
    _sevens(o["ws"][:PAD], "in front of the workspace"), _sevens(o["ws"][PAD + nbytes:], "behind the workspace's documented extent")
    ws = o["ws"][PAD:PAD + nbytes]
    e, xs = _spikes(ws[:M * C], "E"), _spikes(ws[o2:o2 + M * C], "the slice spikes")
    if tape:
        qk = _spikes(ws[o1:o1 + 2 * M * C], "the q | k tape")
        rq, rk, err = DC.attn_check(c, e, qk, xs, xo)
        assert rq["ambiguous"] <= S.AMBIGUOUS_CAP * rq["n"] and rk["ambiguous"] <= S.AMBIGUOUS_CAP * rk["n"], (rq, rk)
        print(f"\nDIGPAR attn {name} q n {rq['n']} ambiguous {rq['ambiguous']} flips {rq['flips']} k ambiguous {rk['ambiguous']} flips {rk['flips']} "
              f"x_err/range {err:.2e}")
    else:
        _sevens(ws[o1:o2], "the q | k region without the tape")
        assert torch.equal(xs.view(c["Tq"], c["rows"], C), c["sproj"].to(torch.uint8)), "slice spikes differ from the oracle"
        DC.range_error(xo, DC.attn_out(c, e), S.RANGE_TOL)
    if o["emit"] is not None:
        em = o["emit"]
        extent = x_rows * C if tape else (x_rows + 80) * C
        _sevens(em[:PAD], "in front of the emitted spikes"), _sevens(em[PAD + extent:], "behind the emission's documented extent")
        if tape:
            got = _spikes(em[PAD:PAD + x_rows * C], "the emitted spikes").view(c["B"], D, c["H"] * c["W"], C)
            want = DC.over_time(DC.emit_neuron(s["emit"], D, 0), xo.view(c["B"], D, c["H"] * c["W"], C))
            assert torch.equal(got, want), f"emitted spikes differ from the neuron on the kernel's own x in {int((got != want).sum())} bytes"
            S.check_rate(want)
    return xo


def _attn_case(monkeypatch, name, env=None):
    s = DC.CASES[name]
    env = s["env"] if env is None else env
    _route(monkeypatch, env)
    c = DC.attn_case(s["C"], s["D"], s["geom"], s["form"], s["cls"])
    layers = _attn_layers(c)
    o = _twice(lambda: _attn_run(c, s, layers, s["tape"]), DC.route(s, env))
    xo = _attn_checks(c, s, o, s["tape"], name)
    other = {**s, "tape": not s["tape"]}
    lines, o2 = _attn_run(c, other, layers, other["tape"], keep_dev=True)
    assert lines == DC.route(other, env), (lines, DC.route(other, env))
    xo2 = _attn_checks(c, other, o2, other["tape"], name)
    assert torch.equal(xo, xo2), "the tape changes the result"
    assert not torch.equal(xo, c["x"].reshape(c["x_rows"], c["Cc"]))
    if s["emit"] is not None:
        # the tiled emission of the production form, handed to the MLP: the x of the MLP on its own first neuron, bit for bit
        prod = o2 if s["tape"] else None
        if prod is None:
            _, prod = _attn_run(c, s, layers, False, keep_dev=True)
        x5, ev = prod["_dev"]
        C, D = c["Cc"], c["D"]
        Ch = DC.handover_Ch(C)
        a1, a2 = 3.0 / C ** 0.5, 2.0 / Ch ** 0.5
        fc1 = _L(DC.rnd((Ch, C), 8901, -a1, a1), *DC.bn(Ch, 8903))
        fc2 = _L(DC.rnd((C, Ch), 8902, -a2, a2), *DC.bn(C, 8905))
        n1, n2 = _np(DC.emit_neuron(s["emit"], D, 0)), _np(DC.mlp_neurons(s["emit"], D, 0)[1])
        xa = hip.ms_mlp(x5.clone(), fc1, fc2, n1, n2, ws=ev, s1_ready=True)
        xb = hip.ms_mlp(x5.clone(), fc1, fc2, n1, n2)
        torch.cuda.synchronize()
        assert torch.equal(xa, xb) and not torch.equal(xa, x5), "the handed-over first spikes differ from the MLP's own"
    tp = (o if s["tape"] else o2)
    return {"x": o["x"], "ws_tape": tp["ws"][PAD:], "emit_tape": tp["emit"]}


# ==================================================================================================== fp32-epilogue products
def _f32_case(monkeypatch, name, env=None):
    s = DC.CASES[name]
    env = s["env"] if env is None else env
    _route(monkeypatch, env)
    k = s["kind"]
    if k == "merge":
        c = DC.merge_case(s["C"], s["D"], s["B"], s["H"], s["W"])
        lin, sp = _L(c["Wr"], c["alpha"], c["beta"]), _dev(c["sp"])
        rows, N = c["ref"].numel() // c["N"], c["N"]
        shape = tuple(c["ref"].shape)

        def call(out):
            assert hip.ms_patch_merge(sp, lin, out=out.view(shape)) is not None, "the merge refused a shape it is built for"
    elif k == "gemm":
        c = DC.gemm_case(s["M"], s["N"], s["K"])
        dg, A = hip.split_weight_i8x3(_dev(c["W"])), _dev(c["A"])
        rows, N = c["M"], c["N"]
        al, be, bi = _dev(c["alpha"]), _dev(c["beta"]), _dev(c["bias"])

        def call(out):
            hip.spike_gemm(A, dg, out, c["M"], N, c["K"], bias=bi, alpha=al, beta=be)
    else:
        c = DC.deconv_case(s["imgs"], s["T"], s["H"], s["W"], s["Cin"], s["Cout"])
        planes, sp = hip.pack_deconv2x2_weight(_dev(c["w"]), c["Cin"]), _dev(c["s"])
        rows, N = c["imgs"] * 4 * c["H"] * c["W"], c["Cout"]
        al, be = _dev(c["alpha"]), _dev(c["beta"])

        def call(out):
            hip.spike_deconv3x3s2(sp, planes, c["imgs"], c["T"], c["H"], c["W"], c["Cin"], N, alpha=al, beta=be, out=out.view(c["imgs"], 2 * c["H"], 2 * c["W"], N))

    def run():
        ob, om = _f32_guarded(rows, N)
        lines, _ = logged(lambda: call(om))
        return lines, {"out": ob.cpu()}
    o = _twice(run, DC.route(s, env))
    _f32_guards_hold(o["out"], rows, "out")
    err = DC.range_error(o["out"][DC.GUARD:DC.GUARD + rows], c["ref"].reshape(rows, N), DC.F32_TOL)
    print(f"\nDIGPAR f32 {name} {DC.route(s, env)[0].split(' ', 3)[3]} err/range {err:.2e}")
    return o


@gpu
def test_k272_is_refused(monkeypatch):
    """K = 272 (K % 16 == 0, not % 32) is a K the row loop's own predicate admits and no entry point passes on: the plain product refuses
    it with SDF_E_SHAPE before any launch (include/sdformerflow_hip.h: "K % 32 == 0"), and writes nothing"""
    _route(monkeypatch, {})
    c = DC.gemm_case(350, 96, 288)
    dg, A = hip.split_weight_i8x3(_dev(c["W"][:, :272])), _dev(c["A"][:, :272])
    ob, om = _f32_guarded(350, 96)
    lines, _ = logged(lambda: hip.spike_gemm(A, dg, om, 350, 96, 272, alpha=_dev(c["alpha"]), beta=_dev(c["beta"])))
    assert lines == [f"rc {hip.E_SHAPE}"], lines
    assert bool(torch.isnan(ob).all())


RUN = {"mlp": _mlp_case, "attn": _attn_case, "merge": _f32_case, "gemm": _f32_case, "deconv": _f32_case}


@gpu
@pytest.mark.parametrize("name", list(DC.CASES))
def test_case(monkeypatch, name):
    t0 = time.time()
    RUN[DC.CASES[name]["kind"]](monkeypatch, name)
    print(f"\nDIGPAR time {name} {time.time() - t0:.2f} s")


FAMILY_CASES = [n for n, s in DC.CASES.items() if DC.other_family(s) is not None]


@gpu
@pytest.mark.parametrize("name", FAMILY_CASES)
def test_families(monkeypatch, name):
    """the same call on two kernel families: other kernels in the launch list, every output bit-equal (x, E, the q | k tape, the slice
    spikes, the hidden spikes, the emit buffers, the merge)"""
    s = DC.CASES[name]
    env2 = DC.other_family(s)
    assert DC.kernels(DC.route(s)) != DC.kernels(DC.route(s, env2)), "the two switch settings name the same kernels"
    a = RUN[s["kind"]](monkeypatch, name)
    b = RUN[s["kind"]](monkeypatch, name, env2)
    _same(a, b, "two kernel families")


# ==================================================================================================== CPU premises (no GPU)
@pytest.mark.parametrize("name", list(DC.PINNED))
def test_derived_routes_equal_the_recorded_pins(name):
    """for the calls tests/test_digit_routes_gpu.py records, the derivation reproduces its literal lines"""
    assert DC.PINNED[name]() == PINS.CASES[name][2]


def test_every_recorded_call_of_this_family_is_restated():
    ours = {n for n in PINS.CASES if not n.startswith("conv_") and n != "gemm_tiled"}      # (out of scope: the convolution and plain-product forms of the small-M kernel)
    assert ours == set(DC.PINNED)


def test_the_cases_reach_every_instantiation():
    """the union of the kernel lines the cases name equals the enumeration of digit_cases.py - a missing instantiation fails by name"""
    assert (len(DC.res_pm_set()), len(DC.res_front_set()), len(DC.wide_pm_set()), len(DC.wide_front_set()), len(DC.smallm_fc2_set())) == (48, 6, 22, 12, 8)
    seen = set()
    for s in DC.CASES.values():
        seen |= DC.kernels(DC.route(s)) | DC.kernels(DC.route({**s, "tape": not s["tape"]}) if "tape" in s else [])
    seen = {k for k in seen if not k.startswith("neuron_kernel")}
    want = DC.every_instantiation()
    assert not want - seen, f"no case reaches {sorted(want - seen)}"
    assert not seen - want, f"the cases name kernels outside the enumeration: {sorted(seen - want)}"
    primary = set()
    for s in DC.CASES.values():
        primary |= DC.kernels(DC.route(s))
    assert not want - primary, f"only a sibling form reaches {sorted(want - primary)}"


def test_the_emitted_neuron_is_of_another_class_than_the_block():
    for kind in ("mlp", "attn"):
        for e in (0, 1, 2):
            assert any(s["kind"] == kind and s["emit"] == e and s["cls"] != e for s in DC.CASES.values()), (kind, e)
    assert all(s["emit"] != s["cls"] for s in DC.CASES.values() if s.get("emit") is not None)


def test_each_shape_sits_where_its_comment_says():
    C, R = DC.CASES, DC.route
    units = lambda n: DC.pm_units(DC.shape_of(C[n])[0], C[n]["D"])
    # units: 35 positions are no multiple of a unit's 8 / 4; 5 units < 8 waves, 9 = 8 + 1; B = 2 with odd HW: a unit straddles the samples
    assert (units("mlp_res192_T10_c0_emit1"), units("mlp_res192_T20_c0_emit1")) == (5, 9) and 35 % 8 and 35 % 4
    assert C["mlp_res192_T10_tape"]["B"] == 2 and (C["mlp_res192_T10_tape"]["H"] * C["mlp_res192_T10_tape"]["W"]) % 8 == 3
    # pick_cb on either side of 600 waves
    for T in (10, 20):
        assert units(f"mlp_wide384_T{T}_c0_cb3") * (1536 // 48) == 608 and f"wide_pm_kernel<{T}, 3, 1, 0, 0>" in R(C[f"mlp_wide384_T{T}_c0_cb3"])[1]
        assert units(f"mlp_wide384_T{T}_cb2_below600") * (1536 // 48) == 576 and f"wide_pm_kernel<{T}, 2, 1, 0, 0>" in R(C[f"mlp_wide384_T{T}_cb2_below600"])[1]
    # pm_ring_grid: passes > 1 inside (256, 1024], one again above, one at most 256
    assert DC.pm_ring(units("mlp_wide384_T10_passes2"), 1536, 3) == (160, 2) and 256 < 32 * DC.cdiv(units("mlp_wide384_T10_passes2"), 4) <= 1024
    assert DC.pm_ring(units("mlp_wide384_T20_above1024"), 1536, 3) == (1088, 1)
    assert DC.pm_ring(units("mlp_wide384_T10_c0_cb3"), 1536, 3) == (160, 1)
    # res_row_ranges: more than one unit per wave, in the product and in the front
    assert DC.res_row_ranges(768 // 32, units("mlp_res192_T20_two_units_per_wave")) == (6, 16)
    assert DC.res_row_ranges(6, units("mlp_res192_T20_c0_emit1"))[1] == 8
    rows = DC.shape_of(C["attn_res512_T10_two_tiles_per_wave"])[1]
    assert rows == 2500 and DC.res_row_ranges(16, DC.cdiv(rows, 16)) == (10, 16)
    # grid8: item counts that are no multiple of 8 (surplus workgroups return)
    for n, kern in (("mlp_res192_T10_c0_emit1", "res_pm_kernel"), ("mlp_res192_T10_c0_smallm_emit1", "smallm_kernel"), ("mlp_res192_T20_smallm", "smallm_kernel")):
        ncg, u = C[n]["C"] // 32, units(n)
        items = ncg * (DC.res_row_ranges(ncg, u)[0] if kern == "res_pm_kernel" else u)
        assert items % 8 and R(C[n])[2].startswith(f"{DC.grid8(items)} ") and kern in R(C[n])[2], (n, items)
    # wide_front_kernel on either side of t5 x nH = 800
    assert DC.cdiv(DC.shape_of(C["attn_wide384_T10_c0_rb4_tape"])[1], 32) * 12 == 948 and "wide_front_kernel<4" in R(C["attn_wide384_T10_c0_rb4_tape"])[1]
    assert DC.cdiv(DC.shape_of(C["attn_wide768_T10_rb2_below800"])[1], 32) * 24 == 768 and "wide_front_kernel<2" in R(C["attn_wide768_T10_rb2_below800"])[1]
    # small-K: K = 256 the last, 288 the first other build an entry point admits
    assert "true, true>" in R(C["gemm_k256"])[0] and "false, true>" in R(C["gemm_k288"])[0] and "false, false>" in R(C["gemm_k288_nostrip"])[0]
    assert "res_pm_kernel<10, 2, 0, 2, false, true>" in R(C["merge_res256_T10_k1024"])[0]
    # slice maps: plain, shifted, padded (entries of -1), N1 = 25 and 81; every row of x is named exactly once
    for g, (B, H, W, window, shift) in DC.GEOM.items():
        m, _ = DC.slice_map(B, 10, H, W, window, shift)
        real = m[m >= 0]
        assert torch.equal(real.sort().values, torch.arange(B * 10 * H * W, dtype=torch.int32))
        assert bool((m < 0).any()) == (g in ("w5s", "w9"))
    assert DC.GEOM["w5"][3][1] * DC.GEOM["w5"][3][2] == 25 and DC.GEOM["w9"][3][1] * DC.GEOM["w9"][3][2] == 81


def _mlp_configs():
    return sorted({(s["C"], s["Ch"], s["D"], s["B"], s["H"], s["W"], s["cls"], s["i"]) for s in DC.CASES.values() if s["kind"] == "mlp"})


def _attn_configs():
    return sorted({(s["C"], s["D"], s["geom"], s["form"], s["cls"]) for s in DC.CASES.values() if s["kind"] == "attn"})


@pytest.mark.parametrize("cfg", _mlp_configs(), ids=lambda c: "-".join(str(v) for v in c))
def test_mlp_premise(cfg):
    """the reference's own spikes pass every step check within the caps; the rates lie in (0.03, 0.97) and differ between the two neurons;
    the digit planes carry each weight within 2^-22 of its row's largest element"""
    c = DC.mlp_case(*cfg)
    rep = S.mlp_check(c, c["s1"], c["s2"], c["out"].float())
    assert rep["flips"] == 0 and rep["ambiguous"] <= S.AMBIGUOUS_CAP * rep["n"]
    r1, r2 = S.check_rate(c["s1"]), S.check_rate(c["s2"])
    assert r1 != r2 and not c["sn1"].same_settings(c["sn2"]) and c["sn1"].cls == c["sn2"].cls == c["cls"]
    for f in (c["fc1"], c["fc2"]):
        assert bool(((f["held"] - f["W"].double()).abs().max(1).values <= 2.0 ** -22 * f["W"].abs().max(1).values.double()).all())
    for e in (0, 1, 2):
        sn = DC.emit_neuron(e, c["D"], cfg[7])
        S.check_rate(DC.over_time(sn, c["out"].float().view(c["B"], c["D"], -1, c["C"])))
        assert sn.cls == e and not sn.same_settings(c["sn1"]) and not sn.same_settings(c["sn2"])


@pytest.mark.parametrize("cfg", _attn_configs(), ids=lambda c: "-".join(str(v) for v in c))
def test_attn_premise(cfg):
    """the reference's own spikes pass every step check; slice, q and k spikes fire inside (0.03, 0.97), the gate inside (0.1, 0.9), at
    different rates; the four neurons differ (sn_k is sn_q in the stacked form, by the entry point's contract)"""
    c = DC.attn_case(*cfg)
    rates = [S.check_rate(t) for t in (c["sproj"], c["q"], c["k"])] + [S.check_rate(c["gate"], 0.1, 0.9)]
    assert len(set(rates)) == 4, rates
    sn = c["sn"]
    assert all(n.cls == c["cls"] for n in sn)
    pairs = [(a, b) for i, a in enumerate(sn) for b in sn[i + 1:]]
    assert sum(a.same_settings(b) for a, b in pairs) == (1 if c["form"] == "stacked" else 0) and (sn[1] is sn[2]) == (c["form"] == "stacked")
    M, C = c["Tq"] * c["rows"], c["Cc"]
    if c["form"] == "stacked":
        qk = torch.cat([c["q"], c["k"]], -1).to(torch.uint8).reshape(-1)
    else:
        qk = torch.cat([c["q"].reshape(-1), c["k"].reshape(-1)]).to(torch.uint8)
    rq, rk, _ = DC.attn_check(c, c["e"].reshape(-1), qk, c["sproj"].to(torch.uint8).reshape(-1), c["out"].float())
    assert rq["flips"] == rk["flips"] == 0 and rq["ambiguous"] <= S.AMBIGUOUS_CAP * rq["n"] and rk["ambiguous"] <= S.AMBIGUOUS_CAP * rk["n"]
    assert 0.03 < float(c["e"].float().mean()) < 0.9
    for k in ("q", "k", "p"):
        W = c["lin"][k]["W"]
        assert bool(((c["held"][k] - W.double()).abs().max(1).values <= 2.0 ** -22 * W.abs().max(1).values.double()).all())
    for e in (0, 1, 2):
        S.check_rate(DC.over_time(DC.emit_neuron(e, c["D"], 0), c["out"].float().view(c["B"], c["D"], -1, C)))


def test_f32_premise():
    """the fp32 of the float64 references is within the 1e-6 the products are held to; the transposed convolution's reference equals the
    product over the 2 x 2 neighbourhood the kernel forms"""
    c = DC.deconv_case(10, 10, 5, 7, 64, 24)
    Mx, _ = DC.deconv_matrix(c["w"], 64)
    s = torch.nn.functional.pad(c["s"].double(), (0, 0, 0, 1, 0, 1))
    H, W = c["H"], c["W"]
    nb = torch.cat([s[:, dh:dh + H, dw:dw + W] for dw in (0, 1) for dh in (0, 1)], -1)          # column block q = dh + 2 dw
    y = (nb @ SC.held_weights(Mx, "i8").t()).view(10, H, W, 2, 2, 24).permute(0, 1, 3, 2, 4, 5).reshape(10, 2 * H, 2 * W, 24)
    y = y * c["alpha"].double() + c["beta"].double()
    assert (y - c["ref"]).abs().max().item() <= 1e-12 * c["ref"].abs().max().item()
    for ref in (c["ref"], DC.merge_case(64, 10, 2, 5, 7)["ref"], DC.gemm_case(350, 96, 288)["ref"]):
        DC.range_error(ref.float(), ref, DC.F32_TOL)
