"""Inputs, float64 references, per-step checks and EXPECTED LAUNCH LINES of tests/test_digit_parity_gpu.py (plain CPU code, no GPU call in
here): the int8 digit-plane kernels of the spiking Swin block - res_pm_kernel / res_front_kernel (csrc/ms_res.hip), wide_pm_kernel /
wide_front_kernel (csrc/ms_wide.hip) and smallm_kernel as fc2 (csrc/ms_smallm.hip) - reached through hip.qk_attn, hip.ms_mlp,
hip.ms_patch_merge and the row-loop forms of hip.spike_gemm and hip.spike_deconv3x3s2.

Every builder is cached: the tests share one reference per case, and nothing mutates what a builder returned.

The references are float64 on the value the digit planes carry (spike_conv_cases.held_weights(W, "i8") - `_weff` of test_ms_wide_gpu.py
restated on the CPU; the GPU test compares it with the device's planes).  The step checks and their caps are stage0_cases.py's
(mlp_check, qk_check: tests/replay.py's delta rule, 0 unexplained, <= 1e-4 ambiguous, <= 2e-4 flipped, 1e-5 of the range); the fp32
products (merge, plain product, transposed convolution) are exact integer sums: 1e-6 of the range.

The launch lines ("workgroups threads LDS-bytes kernel<args>", routes_common.logged's notation) are DERIVED here from the dispatch code
restated below - each rule quotes its source - and not recorded from a run; PINNED restates the calls tests/test_digit_routes_gpu.py
records, and the derivation must reproduce those literal lines (test_derived_routes_equal_the_recorded_pins).

Neurons.  Wherever a call takes several they get DIFFERENT settings of one class (stage0_cases.py's rule): the attention's four through
stage0_cases.qk_neurons (sn_k is sn_q in the stacked form, by the entry point's contract), sn1 / sn2 through mlp_neurons; the neuron
a call EMITS for (epilogue 3) is of another class than the block's, so every NK of epilogue 3 is reached from a foreign block.

Out of scope: the convolution and plain-product forms of smallm_kernel and wide_pm_kernel<T, 2, 4, 0> + wide_reduce_kernel
(test_smallm_gpu.py, test_wide_conv_gpu.py: the obvious follow-up), and shapes whose index arithmetic passes 2^31.
"""
import functools

import torch

import spike_conv_cases as SC
import stage0_cases as S
from stage0_cases import CLASS2, Neuron, check_rate, check_report, neuron, slice_map        # noqa: F401 (re-exported to the test file)
from sdformerflow_amd.synthetic import synth_uniform as rnd

GUARD = 64                       # guard rows on each side of x / of an fp32 output
F32_TOL = 1e-6                   # exact integer sums + one fp32 epilogue, against the range (test_ms_wide_gpu.py, test_smallm_gpu.py)
KRING = {"SDF_RES_MAXC": "191"}  # the K-ring kernels from 192 channels on
MINC64 = {"SDF_RES_MINC": "64"}  # the row loop from 64 channels on
NOSTRIP = {"SDF_RES_STRIP": "0"}
TF = {True: "true", False: "false"}


# ==================================================================================================== the instantiations
def res_pm_set():
    """ms_res.hip:657  `if constexpr ((e == 2 || (a == 0 && st == 0)) && (e != 2 || n == 0))` over T 10 / 20, AM 0 / 2 / 3, EPI 1 / 2 / 3,
    NK 0 / 1 / 2, STRIP, small-K (launch_res_pm's six sdf_dispatch lists): 48"""
    return {f"res_pm_kernel<{T}, {e}, {n}, {a}, {TF[sk]}, {TF[st]}>" for T in (10, 20) for a in (0, 2, 3) for e in (1, 2, 3) for n in (0, 1, 2)
            for st in (False, True) for sk in (False, True) if (e == 2 or (a == 0 and not st)) and (e != 2 or n == 0)}


def res_front_set():
    """ms_res.hip:685-687  sdf_dispatch(SdfList<0, 1, 2>, nk) x sdf_dispatch(SdfList<1, 0>, keep), no condition: 6"""
    return {f"res_front_kernel<{n}, {TF[k]}>" for n in (0, 1, 2) for k in (False, True)}


def wide_pm_set():
    """ms_wide.hip:771  `if constexpr ((c == 2 || e == 1) && (e != 2 || n == 0))` over T 10 / 20, CB 3 / 2, EPI 1 / 2 / 3, NK: 20; and
    ms_wide.hip:884 the merge form wide_pm_kernel<t, 2, 2, 0, 2>: 2"""
    return {f"wide_pm_kernel<{T}, {c}, {e}, {n}, 0>" for T in (10, 20) for c in (2, 3) for e in (1, 2, 3) for n in (0, 1, 2)
            if (c == 2 or e == 1) and (e != 2 or n == 0)} | {f"wide_pm_kernel<{T}, 2, 2, 0, 2>" for T in (10, 20)}


def wide_front_set():
    """ms_wide.hip:946-948  SdfList<4, 2> x SdfList<0, 1, 2> x SdfList<1, 0>, no condition: 12"""
    return {f"wide_front_kernel<{rb}, {n}, {TF[k]}>" for rb in (2, 4) for n in (0, 1, 2) for k in (False, True)}


def smallm_fc2_set():
    """ms_smallm.hip:550-551  launch_smallm<0, true>(T 10 / 20, CB 2, EPI of SdfList<2, 1, 3>) with epi = emit ? 3 : 2 and
    nk = emit ? class : 0: 8"""
    return {f"smallm_kernel<{T}, {e}, {n}, 0, true, 2>" for T in (10, 20) for e, n in ((2, 0), (3, 0), (3, 1), (3, 2))}


def every_instantiation():
    return res_pm_set() | res_front_set() | wide_pm_set() | wide_front_set() | smallm_fc2_set()


# ==================================================================================================== the dispatch code, restated
def cdiv(a, b):
    return -(-a // b)


def pm_units(positions, T):
    """digit_host.h:14  a wave owns 80 rows = 4 * (20 / T) positions x T steps"""
    return cdiv(positions, 4 * (20 // T))


def grid8(items):
    """digit_host.h:22  one workgroup per item, rounded up to a multiple of 8 (the surplus workgroups return)"""
    return cdiv(items, 8) * 8


def res_row_ranges(cols, n):
    """digit_host.h:48  the smallest r units per wave for which cols x ranges of 8 r units fit 256 compute units -> (ranges, 8 r)"""
    r = 1
    while cols * cdiv(n, 8 * r) > 256:
        r += 1
    return cdiv(n, 8 * r), 8 * r


def pm_ring(units, N, cb):
    """digit_host.h:32 pm_ring_grid -> (workgroups, passes): 4 units per row group; up to four rounds run as one"""
    nrg, ncg = cdiv(units, 4), N // (16 * cb)
    every = ncg * nrg
    passes = cdiv(every, 256) if 256 < every <= 1024 else 1
    return grid8(ncg * cdiv(nrg, passes)), passes


def pick_cb(units, N, cbs):
    """ms_wide.hip:744  the widest tile that still leaves >= 600 waves, else the narrowest"""
    for cb in reversed(cbs):
        if N % (16 * cb) == 0 and units * (N // (16 * cb)) >= 600:
            return cb
    return next(cb for cb in cbs if N % (16 * cb) == 0)


def s_pitch(nbytes):
    """wide_common.h:103"""
    return nbytes + 16 if ((nbytes + 16) // 4) % 8 == 4 else nbytes + 32


def res_wbytes(K, BN):
    """ms_res.hip:64-65  the resident digits: 3 planes x (K / 16 rounded up to 4) pieces x BN columns x 16 bytes"""
    return 3 * (((K >> 4) + 3) & ~3) * BN * 16


def res_pm_lds(K, epi, nk):
    """ms_res.hip:608  digits + (neuron epilogues: 8 waves' byte tiles) + 8 x 80 row offsets + 32 x 16 + (PSN: PSN_TABLE(20) floats) +
    (epilogue 2: the strips, 8 waves x RBW = 5 KB)"""
    b = res_wbytes(K, 32) + (8 * 80 * s_pitch(32) if epi & 1 else 0) + 8 * 80 * 4 + 32 * 16
    return b + (420 * 4 if nk == 1 else 0) + (8 * 5 * 1024 if epi == 2 else 0)


def res_stage_ok(C, env, merge=False):
    """ms_wide.hip:805-819  SDF_RES=0: off; the merge up to 256 channels; else SDF_RES_MINC (32..192, default 128) <= C <= SDF_RES_MAXC (768)"""
    if env.get("SDF_RES") == "0" or C < 64 or C % 32:
        return False
    if merge:
        return C <= 256
    return int(env.get("SDF_RES_MINC", 128)) <= C <= int(env.get("SDF_RES_MAXC", 768))


def res_pm_line(positions, T, N, K, epi, nk, env, am=0, a_tiled=False, zsrc=False):
    """ms_res.hip:630 launch_res_pm (after res_pm_takes, ms_res.hip:620: K % 16, 32 <= K <= 1024, N % 32, with zsrc K % 32)"""
    assert K % 16 == 0 and 32 <= K <= 1024 and N % 32 == 0 and not (zsrc and K % 32), (N, K)
    units, ncg = pm_units(positions, T), N // 32
    nrg, _ = res_row_ranges(ncg, units)
    nk = nk if epi & 1 else 0
    # ms_res.hip:603-606, :647  strip = epi == 2 && SDF_RES_STRIP != 0 && (merged / transposed operands || plain row-major rows)
    strip = epi == 2 and env.get("SDF_RES_STRIP") != "0" and (am != 0 or (not a_tiled and not zsrc))
    return f"{grid8(ncg * nrg)} 512 {res_pm_lds(K, epi, nk)} res_pm_kernel<{T}, {epi}, {nk}, {am}, {TF[K <= 256]}, {TF[strip]}>"


def pm_line(positions, T, N, K, epi, nk, res_stage, env, a_tiled=False, zsrc=False):
    """ms_wide.hip:752 launch_pm: the row loop where res_pm_takes, else the K ring with pick_cb's column blocks"""
    if res_stage and env.get("SDF_RES") != "0" and K % 16 == 0 and 32 <= K <= 1024 and N % 32 == 0 and not (zsrc and K % 32):
        return res_pm_line(positions, T, N, K, epi, nk, env, 0, a_tiled, zsrc)
    units = pm_units(positions, T)
    cb = pick_cb(units, N, (2, 3) if epi == 1 else (2,))
    wgs, _ = pm_ring(units, N, cb)
    return f"{wgs} 256 0 wide_pm_kernel<{T}, {cb}, {epi}, {0 if epi == 2 else nk}, 0>"


def neuron_line(T, per_step):
    """neuron.hip:336  one thread per four values of a step"""
    return f"{cdiv(cdiv(per_step, 4), 256)} 256 0 neuron_kernel<{T}>"


def smallm_fc2_takes(C, Ch, D, positions, tiled, env):
    """ms_smallm.hip:526 smallm_fc2_supports: fragment-order digits, at most 64 x 80 tokens, tiles that fit the chip in one round"""
    if not tiled or env.get("SDF_SMALLM") == "0" or env.get("SDF_SMALLM_FC2") == "0" or Ch % 64 or C % 32:
        return False
    return positions * D <= 64 * 80 and (pm_units(positions, D) * (C // 32) <= 512 or env.get("SDF_SMALLM_FC2") == "2")


def route_mlp(C, Ch, D, positions, cls, emit, tape, tiled=False, env={}, s1_ready=False):
    """hip.ms_mlp on the wide-stage kernels (qk_attn.hip:203, ms_wide.hip:844 launch_ms_wide_mlp): [SN1] -> fc1 (epilogue 1, SN2's class) ->
    fc2 (epilogue 2, or 3 with the emitted neuron's class) on the small-M kernel, the row loop or the K ring.  `cls`: the block's
    class, `emit`: the emitted neuron's class or None."""
    res = res_stage_ok(C, env) and C <= 192 and Ch % 32 == 0 and Ch <= 768
    assert res or (C >= 192 and C % 64 == 0 and Ch % 64 == 0 and Ch % 96 == 0), "ms_wide_mlp_supports (ms_wide.hip:828) refuses this"
    small = smallm_fc2_takes(C, Ch, D, positions, tiled, env)
    lines = [] if s1_ready else [neuron_line(D, positions * C)]
    lines.append(pm_line(positions, D, Ch, C, 1, cls, res_stage_ok(C, env), env, a_tiled=s1_ready and not tape))
    epi, nk = (2, 0) if emit is None else (3, emit)
    if small:
        lines.append(f"{grid8((C // 32) * pm_units(positions, D))} 256 0 smallm_kernel<{D}, {epi}, {nk}, 0, true, 2>")
    else:
        lines.append(pm_line(positions, D, C, Ch, epi, nk, res_stage_ok(C, env), env, a_tiled=not tape))
    return lines


def route_attn(C, D, positions, rows, cls, emit, tape, env={}):
    """hip.qk_attn with x_src on the wide-stage kernels (qk_attn.hip:153): slice neuron over the T' = 2 steps -> the front kernel (ms_wide.hip:914:
    the row loop for 64 <= C <= 512 where the stage takes it, ms_res.hip:671-693; else 32-token tiles while t5 * nH >= 800, else 16) ->
    the projection through launch_pm with the scramble map (ms_wide.hip:954).  `rows` = B_ N1."""
    nH = C // 32
    res = res_stage_ok(C, env) and C <= 192
    assert res or (C >= 192 and C % 64 == 0), "ms_wide_attn_supports (ms_wide.hip:888) refuses this"
    lines = [neuron_line(2, rows * C)]
    if res_stage_ok(C, env) and 64 <= C <= 512:
        nrg, _ = res_row_ranges(nH, cdiv(rows, 16))
        lds = res_wbytes(C, 64) + 8 * 32 * s_pitch(96 if tape else 32)
        lines.append(f"{grid8(nrg * nH)} 512 {lds} res_front_kernel<{cls}, {TF[tape]}>")
    else:
        t5, t2 = cdiv(rows, 32), cdiv(rows, 16)
        big = t5 * nH >= 800
        lines.append(f"{grid8(cdiv(t5 if big else t2, 4) * nH)} 256 0 wide_front_kernel<{4 if big else 2}, {cls}, {TF[tape]}>")
    epi, nk = (2, 0) if emit is None else (3, emit)
    lines.append(pm_line(positions, D, C, C, epi, nk, res_stage_ok(C, env), env, zsrc=True))
    return lines


def route_merge(C, N, D, positions, env={}):
    """hip.ms_patch_merge (ms_wide.hip:877): the row loop up to 256 channels (AM 2, K = 4 C), else the K ring's merge form, two column blocks"""
    if res_stage_ok(C, env, merge=True):
        return [res_pm_line(positions, D, N, 4 * C, 2, 0, env, am=2)]
    assert C % 64 == 0
    return [f"{pm_ring(pm_units(positions, D), N, 2)[0]} 256 0 wide_pm_kernel<{D}, 2, 2, 0, 2>"]


def route_gemm(M, N, K, env={}):
    """hip.spike_gemm on row-major digit planes (spike_gemm.hip:461-474): 10 "steps" x M / 10 "positions" on the row loop"""
    return [res_pm_line(M // 10, 10, N, K, 2, 0, env)]


def route_deconv(imgs, T, H, W, Cin, Cout, env={}):
    """hip.spike_deconv3x3s2 off the last decoder level's shape (spike_gemm.hip:597-613): one product over the 2 x 2 neighbourhood, AM 3"""
    return [res_pm_line((imgs // T) * H * W, T, 4 * Cout, 4 * Cin, 2, 0, env, am=3)]


# ---- the calls tests/test_digit_routes_gpu.py records, restated (lif: class 0, psn: 1, lif_hard / if: 2; its emitted neuron is the block's)
PINNED = {
    "mlp_res_lif": lambda: route_mlp(192, 768, 10, 35, 0, None, False),
    "mlp_res_psn_T20_emit_tape": lambda: route_mlp(192, 768, 20, 35, 1, 1, True),
    "mlp_res_hard_tape": lambda: route_mlp(192, 768, 10, 35, 2, None, True),
    "mlp_res384_if_emit_smallm_fc2": lambda: route_mlp(384, 1536, 10, 35, 2, 2, False, tiled=True),
    "mlp_res384_lif_T20_smallm_fc2": lambda: route_mlp(384, 1536, 20, 9, 0, None, False, tiled=True),
    "mlp_wide_lif_cb3": lambda: route_mlp(384, 1536, 10, 192, 0, None, False, env=KRING),
    "mlp_wide_psn_T20_cb2_emit": lambda: route_mlp(384, 1536, 20, 35, 1, 1, False, env=KRING),
    "mlp_wide_hard_cb2_emit": lambda: route_mlp(384, 1536, 10, 35, 2, 2, False, env=KRING),
    "mlp_default384_lif": lambda: route_mlp(384, 1536, 10, 35, 0, None, False),
    "attn_res_lif_tape_emit": lambda: route_attn(192, 10, 25, 125, 0, 0, True),
    "attn_res_psn_T20": lambda: route_attn(192, 20, 25, 250, 1, None, False),
    "attn_res_if_emit": lambda: route_attn(192, 10, 25, 125, 2, 2, False),
    "attn_wide_lif_tape": lambda: route_attn(384, 10, 25, 125, 0, None, True, env=KRING),
    "attn_wide_hard_T20_emit": lambda: route_attn(384, 20, 25, 250, 2, 2, False, env=KRING),
    "attn_wide_psn_emit": lambda: route_attn(384, 10, 25, 125, 1, 1, False, env=KRING),
    "merge_res_c64_T20": lambda: route_merge(64, 128, 20, 12),
    "merge_res_c96": lambda: route_merge(96, 192, 10, 24),
    "merge_wide_c320": lambda: route_merge(320, 640, 10, 12),
    "gemm_rowmajor_k128": lambda: route_gemm(350, 96, 128),
    "gemm_rowmajor_k384": lambda: route_gemm(350, 96, 384),
    "deconv_c64": lambda: route_deconv(10, 10, 5, 7, 64, 32),
    "deconv_c96_T20": lambda: route_deconv(20, 20, 5, 7, 96, 8),
}


# ==================================================================================================== neurons
VTH = {"lif": 0.1, "plif": 0.12, "lif_hard": 0.1, "lif_vr": 0.12, "lif_tau3": 0.08, "if": 0.4, "psn": 0.0}       # stage0_cases.MLP_VTH


def mlp_neurons(cls, D, i):
    """(sn1, sn2): two settings of the class; lif / plif swap and the class-2 pair rotates with i"""
    names = {0: (("lif", "plif"), ("plif", "lif"))[i % 2], 1: ("psn", "psn"), 2: (CLASS2[i % 4], CLASS2[(i + 2) % 4])}[cls]
    return neuron(names[0], VTH[names[0]], D, 20), neuron(names[1], 1.25 * VTH[names[1]], D, 21)


def emit_neuron(cls, D, i):
    """the neuron a call emits for: its own class, a setting none of the block's neurons has (threshold 2 x the table's; PSN: its own matrix)"""
    name = {0: ("plif", "lif")[i % 2], 1: "psn", 2: CLASS2[(i + 1) % 4]}[cls]
    return neuron(name, 2.0 * VTH[name], D, 22)


# ==================================================================================================== MLP
@functools.lru_cache(maxsize=None)
def mlp_case(C, Ch, D, B, H, W, cls, i=0):
    """The keys of stage0_cases.mlp_case (so that its mlp_check / mlp_pre2 / mlp_steps serve) with the weights as the digit planes hold
    them, + the reference's own chain: s2 (ntok, Ch) and out (ntok, C) float64."""
    seed = 8100 + 11 * D + C + 3 * B + 5 * H + W
    sn1, sn2 = mlp_neurons(cls, D, i)
    x = rnd((B, D, H, W, C), seed, -0.5, 1.0)
    a1, a2 = 3.0 / C ** 0.5, 2.0 / Ch ** 0.5                    # (stage0_cases' +-0.3 at K = 96 and +-0.1 at K = 384, kept alike in the sum)
    fc1 = {"W": rnd((Ch, C), seed + 1, -a1, a1), "alpha": rnd((Ch,), seed + 3, 0.5, 1.5), "beta": rnd((Ch,), seed + 4, -0.2, 0.2)}
    fc2 = {"W": rnd((C, Ch), seed + 2, -a2, a2), "alpha": rnd((C,), seed + 5, 0.5, 1.5), "beta": rnd((C,), seed + 6, -0.2, 0.2)}
    for f in (fc1, fc2):
        f["held"] = SC.held_weights(f["W"], "i8")
    ntok = B * D * H * W
    s1 = sn1.ref(x.permute(1, 0, 2, 3, 4).contiguous()).permute(1, 0, 2, 3, 4).reshape(ntok, C).to(torch.uint8)
    c = {"B": B, "D": D, "H": H, "W": W, "C": C, "Ch": Ch, "ntok": ntok, "cls": cls, "x": x, "fc1": fc1, "fc2": fc2, "sn1": sn1, "sn2": sn2, "s1": s1}
    s2 = sn2.ref(S.mlp_pre2(c, s1)).view(D, B, H * W, Ch).permute(1, 0, 2, 3).reshape(ntok, Ch).to(torch.uint8)
    c["s2"], c["out"] = s2, mlp_out(c, s2)
    return c


def mlp_out(c, s2):
    """x + BN2(s2 W2^T) in float64 on the hidden spikes `s2` (ntok, Ch)"""
    return c["x"].reshape(c["ntok"], c["C"]).double() + (s2.double() @ c["fc2"]["held"].t()) * c["fc2"]["alpha"].double() + c["fc2"]["beta"].double()


def over_time(sn, x5):
    """SN over dim 1 (the D steps) of a (B, D, ...) fp32 tensor -> u8 of the same shape"""
    p = (1, 0) + tuple(range(2, x5.dim()))
    return sn.ref(x5.permute(*p).contiguous()).permute(*p).contiguous().to(torch.uint8)


def mlp_ws_bytes(ntok, C, Ch):
    """qk_attn.hip:184 sdf_ms_mlp_workspace_bytes: + 80 rows each - the tiled hand-over layout rounds the rows up to whole 80-row units"""
    return cdiv((ntok + 80) * C, 256) * 256 + (ntok + 80) * Ch


# ==================================================================================================== attention
GEOM = {   # (B, H, W, window, shift)
    "w5": (1, 5, 5, (2, 5, 5), (0, 0, 0)),        # N1 = 25 (the wide form wants N1 >= 24), one spatial window, plain map: 25 positions - no
                                                  # multiple of 8 or 4 - in 4 (T = 10) / 7 (T = 20) units: fewer than a workgroup's 8 waves
    "w5s": (2, 7, 9, (2, 5, 5), (1, 2, 2)),       # shifted, 7 x 9 padded to 10 x 10 (entries of -1), B = 2 with HW = 63 odd: a unit straddles the samples
    "w9": (1, 11, 13, (2, 9, 9), (1, 4, 4)),      # N1 = 81, shifted, padded to 18 x 18
    "w5big": (1, 20, 25, (2, 5, 5), (0, 0, 0)),   # 20 spatial windows: at D = 10 2 500 rows - t5 = 79 token tiles, 79 x 12 heads >= 800 at C = 384 (RB = 4),
                                                  # and 157 16-token tiles x 16 heads at C = 512: 16 x ceil(157 / 8) = 320 > 256, two tiles' worth per wave
    "w5mid": (1, 10, 20, (2, 5, 5), (0, 0, 0)),   # 8 spatial windows: at D = 10 1 000 rows, t5 x nH = 32 x 24 = 768 < 800 at C = 768 (RB = 2 just below the rule)
}


@functools.lru_cache(maxsize=None)
def attn_case(C, D, geom, form, cls):
    """The keys of stage0_cases.qk_case (its qk_pre / qk_gate_of / qk_check / qk_tape serve) with the weights as the digit planes hold them,
    + the reference's own chain: q, k, gate, e (Tq, rows, C) u8 and out (x_rows, C) float64."""
    B, H, W, window, shift = GEOM[geom]
    Tq, N1, nH = window[0], window[1] * window[2], C // 32
    seed = 8300 + C + 7 * N1 + 3 * cls + 11 * D + H + (1 if form == "stacked" else 0)
    x = rnd((B, D, H, W, C), seed, -0.5, 1.0)
    a = 2.4 / C ** 0.5                                          # (stage0_cases' +-0.2 at C = 144, kept alike in the sum)
    lin = {k: {"W": rnd((C, C), seed + 10 * i + 1, -a, a), "alpha": rnd((C,), seed + 10 * i + 2, 0.5, 1.5),
               "beta": rnd((C,), seed + 10 * i + 3, -0.2, 0.2)} for i, k in enumerate(("q", "k", "p"))}
    lin["p"]["bias"] = rnd((C,), seed + 40, -0.1, 0.1)
    pe = rnd((Tq * N1, C), seed + 41, -0.3, 0.3)
    m, B_ = slice_map(B, D, H, W, window, shift)
    rows = B_ * N1
    sn = S.qk_neurons(cls, form, C)
    xg = torch.zeros((Tq * rows, C))
    xg[m >= 0] = x.reshape(-1, C)[m[m >= 0].long()]
    sproj = sn[0].ref(xg.view(Tq, rows, C).contiguous())
    held = {k: SC.held_weights(lin[k]["W"], "i8") for k in ("q", "k", "p")}      # (per-row scales: stacking q over k changes no digit)
    c = {"Cc": C, "nH": nH, "Tq": Tq, "N1": N1, "B_": B_, "rows": rows, "B": B, "D": D, "H": H, "W": W, "window": window, "shift": shift,
         "x_rows": B * D * H * W, "form": form, "cls": cls, "x": x, "lin": lin, "pe": pe, "map": m, "held": held, "sproj": sproj, "sn": sn}
    c["pre_q"], c["pre_k"] = S.qk_pre(c, sproj)
    c["q"], c["k"] = sn[1].ref(c["pre_q"]), sn[2].ref(c["pre_k"])
    c["gate"] = S.qk_gate_of(c, c["q"])
    c["e"] = (c["k"].view(Tq, rows, nH, 32) * c["gate"][..., None]).view(Tq, rows, C).to(torch.uint8)
    c["out"] = attn_out(c, c["e"])
    return c


def attn_out(c, e):
    """x + scatter(BN(Z Wp^T + b)) in float64, Z = the gated spikes `e` (Tq, rows, C) read through the reference's raw head reshape
    (Spiking_swin_transformer3D.py:706-717; test_ms_wide_gpu.py step (d)) -> (x_rows, C)"""
    C, M, p = c["Cc"], c["Tq"] * c["rows"], c["lin"]["p"]
    Z = e.reshape(c["B_"], c["nH"], c["Tq"], c["N1"], 32).permute(2, 0, 3, 1, 4).reshape(M, C).double()
    Y = ((Z @ c["held"]["p"].t()) + p["bias"].double()) * p["alpha"].double() + p["beta"].double()
    ref = c["x"].reshape(c["x_rows"], C).double().clone()
    ok = c["map"] >= 0
    ref[c["map"][ok].long()] += Y[ok]
    return ref


def attn_ws_bytes(c):
    """qk_attn.hip:119 sdf_qk_attn_workspace_bytes: E (first the slice spikes' place), q | k, the slice spikes -> (total, the three offsets)"""
    M, C = c["Tq"] * c["rows"], c["Cc"]
    o1 = cdiv(M * C, 256) * 256
    o2 = o1 + cdiv(2 * M * C, 256) * 256
    return o2 + M * C, (0, o1, o2)


def attn_check(c, e, qk, xs, xo):
    """The oracle, step by step, on what the kernels left: slice spikes bit-equal; q | k delta-consistent (positional term on k); E bit-equal
    to k AND SN2_q(head sums of the kernel's own q); the output through the head scramble and the scatter within 1e-5 of its range on the
    kernel's own E.  -> (q's report, k's report, the output's error against the range)"""
    Tq, rows, C = c["Tq"], c["rows"], c["Cc"]
    want = c["sproj"].to(torch.uint8)
    assert torch.equal(xs.view(Tq, rows, C), want), f"slice spikes differ from the oracle in {int((xs.view(Tq, rows, C) != want).sum())} bytes"
    q, k = S.qk_tape(c, qk)
    check_rate(q), check_rate(k)
    e = e.view(Tq, rows, C)
    rq, rk = S.qk_check(c, q, k, e)
    return rq, rk, range_error(xo.reshape(c["x_rows"], C), attn_out(c, e), S.RANGE_TOL)


def range_error(got, ref, tol):
    assert not torch.isnan(got).any(), "NaN left where a result belongs"
    err, rng = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    assert err <= tol * rng, (err, rng)
    return err / rng


# ==================================================================================================== fp32-epilogue products
def bn(N, seed):
    return rnd((N,), seed, 0.5, 1.5), rnd((N,), seed + 1, -0.2, 0.2)


@functools.lru_cache(maxsize=None)
def merge_case(C, D, B, H, W):
    """spikes (B, D, H, W, C) at rate 0.3, the reduction 4 C -> 2 C; ref = BN(cat_2x2(S) W^T) float64 in the reference's order
    (Spiking_swin_transformer3D.py:960-972: zero padding to even sizes, x0..x3 = (0,0), (1,0), (0,1), (1,1))"""
    N, seed = 2 * C, 8500 + C + D + 3 * B + 5 * H + W
    sp = (rnd((B, D, H, W, C), seed, 0.0, 1.0) < 0.3).to(torch.uint8)
    Wr = rnd((N, 4 * C), seed + 1, -0.08, 0.08)
    alpha, beta = bn(N, seed + 2)
    s = torch.nn.functional.pad(sp.double(), (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([s[:, :, 0::2, 0::2], s[:, :, 1::2, 0::2], s[:, :, 0::2, 1::2], s[:, :, 1::2, 1::2]], -1)
    ref = (cat @ SC.held_weights(Wr, "i8").t()) * alpha.double() + beta.double()
    return {"C": C, "N": N, "D": D, "B": B, "H": H, "W": W, "sp": sp, "Wr": Wr, "alpha": alpha, "beta": beta, "ref": ref,
            "positions": B * cdiv(H, 2) * cdiv(W, 2)}


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K):
    """A (M, K) at rate 0.3, W (N, K), bias, BN; ref = BN(A W^T + bias) float64 (test_plain_product_on_row_major_digits)"""
    seed = 8600 + M + N + K
    A = (rnd((M, K), seed, 0.0, 1.0) < 0.3).to(torch.uint8)
    Wm, bias = rnd((N, K), seed + 1, -0.1, 0.1), rnd((N,), seed + 4, -0.1, 0.1)
    alpha, beta = bn(N, seed + 2)
    ref = ((A.double() @ SC.held_weights(Wm, "i8").t()) + bias.double()) * alpha.double() + beta.double()
    return {"M": M, "N": N, "K": K, "A": A, "W": Wm, "bias": bias, "alpha": alpha, "beta": beta, "ref": ref}


def deconv_matrix(w, cin_pad):
    """hip.pack_deconv2x2_weight's (4 Cout, 4 cin_pad) matrix, on the CPU: row (2 py + px) Cout + co, column (dh + 2 dw) cin_pad + c"""
    Cin, Cout = w.shape[:2]
    Mx = torch.zeros((4 * Cout, 4 * cin_pad))
    tap = {(0, 0): 1, (1, 0): 2, (1, 1): 0}                      # (output parity, input offset) -> kernel index
    for (py, dh), ky in tap.items():
        for (px, dw), kx in tap.items():
            q, cl = dh + 2 * dw, 2 * py + px
            Mx[cl * Cout:(cl + 1) * Cout, q * cin_pad:q * cin_pad + Cin] = w[:, :, ky, kx].t()
    return Mx, tap


@functools.lru_cache(maxsize=None)
def deconv_case(imgs, T, H, W, Cin, Cout):
    """s (imgs, H, W, Cin) at rate 0.3; ref = BN(conv_transpose2d(3, 2, 1, 1)) in float64 with every kernel tap as the digit planes of the
    product's matrix hold it (each tap stands in exactly one block of the matrix) -> (imgs, 2H, 2W, Cout)"""
    seed = 8700 + imgs + T + H + W + Cin + Cout
    s = (rnd((imgs, H, W, Cin), seed, 0.0, 1.0) < 0.3).to(torch.uint8)
    w = rnd((Cin, Cout, 3, 3), seed + 1, -0.3, 0.3)
    alpha, beta = bn(Cout, seed + 2)
    Mx, tap = deconv_matrix(w, Cin)
    held = SC.held_weights(Mx, "i8")
    wh = torch.zeros((Cin, Cout, 3, 3), dtype=torch.float64)
    for (py, dh), ky in tap.items():
        for (px, dw), kx in tap.items():
            q, cl = dh + 2 * dw, 2 * py + px
            wh[:, :, ky, kx] = held[cl * Cout:(cl + 1) * Cout, q * Cin:(q + 1) * Cin].t()
    y = torch.nn.functional.conv_transpose2d(s.permute(0, 3, 1, 2).double(), wh, None, 2, 1, 1).permute(0, 2, 3, 1)
    return {"imgs": imgs, "T": T, "H": H, "W": W, "Cin": Cin, "Cout": Cout, "s": s, "w": w, "alpha": alpha, "beta": beta,
            "ref": (y * alpha.double() + beta.double()).contiguous()}


# ==================================================================================================== the cases
def _mlp(C, D, cls, emit=None, tape=False, tiled=False, env={}, B=1, HW=(5, 7), Ch=None, i=0):
    return {"kind": "mlp", "C": C, "Ch": Ch or 4 * C, "D": D, "B": B, "H": HW[0], "W": HW[1], "cls": cls, "emit": emit, "tape": tape, "tiled": tiled,
            "env": dict(env), "i": i}


def _attn(C, D, cls, emit=None, tape=False, form="separate", geom="w5", env={}):
    return {"kind": "attn", "C": C, "D": D, "geom": geom, "form": form, "cls": cls, "emit": emit, "tape": tape, "env": dict(env)}


def handover_Ch(C):
    """a hidden width the wide-stage MLP takes at C channels (ms_wide_mlp_supports beyond 192 channels: Ch % 64 == 0 and Ch % 96 == 0)"""
    return 4 * C if C <= 192 or (4 * C) % 96 == 0 else 3 * C


def _cases():
    c = {}
    # ---- MLP.  5 x 7 = 35 positions: no multiple of the 8 (T = 10) / 4 (T = 20) of a unit; 5 units - fewer than the 8 waves - and 9 = 8 + 1 units
    for T in (10, 20):
        for cls in (0, 1, 2):
            e1, e2 = (cls + 1) % 3, (cls + 2) % 3
            # row loop, C = 192: fc1 K = 192 (small-K), fc2 K = 768 with epilogue 3 for a neuron of another class
            c[f"mlp_res192_T{T}_c{cls}_emit{e1}"] = _mlp(192, T, cls, e1, tape=cls == 1, i=cls)
            # row loop from 64 channels: fc1 K = 64 (ONE 64-deep step), fc2 K = 256 (the last small-K build) with epilogue 3
            c[f"mlp_res64_T{T}_c{cls}_emit{e2}"] = _mlp(64, T, cls, e2, tape=cls == 0, env=MINC64, i=cls + 1)
            # C = 384: fc1 K = 384 on the row loop (not small-K), fc2 K = 1536 on the small-M kernel
            c[f"mlp_res384_T{T}_c{cls}_smallm_emit{e2}"] = _mlp(384, T, cls, e2, tiled=True, i=cls)
            # C = 192: fc2 K = 768 on the small-M kernel, which the ROW LOOP serves with the small-M kernel off (test_families: bit-equal);
            # 6 column tiles x 5 (T = 10) / 9 (T = 20) units = 30 / 54 workgroups: no multiples of 8, the surplus ones return
            c[f"mlp_res192_T{T}_c{cls}_smallm_emit{e1}"] = _mlp(192, T, cls, e1, tiled=True, tape=cls == 2, i=cls + 2)
            # K ring, two column blocks (9 or 5 units: far below 600 waves): fc1 K = 384 = three chunks, fc2 K = 1536
            c[f"mlp_wide384_T{T}_c{cls}_emit{e1}"] = _mlp(384, T, cls, e1, env=KRING, i=cls + 1)
            # K ring, three column blocks: 19 units x 1536 / 48 = 608 >= 600 (T = 10: 147 = 7 x 21 positions / 8; T = 20: 75 = 5 x 15 / 4)
            c[f"mlp_wide384_T{T}_c{cls}_cb3"] = _mlp(384, T, cls, tape=cls == 2, env=KRING, HW=(7, 21) if T == 10 else (5, 15), i=cls)
        # fc2 with the fp32 epilogue: tiled hidden spikes (no tape) and row-major ones (tape: the strip build), K = 768 and K = 256 (small-K);
        # B = 2 with HW = 35 odd: a unit straddles the two samples
        c[f"mlp_res192_T{T}_tape"] = _mlp(192, T, 0, tape=True, B=2, i=1)
        c[f"mlp_res192_T{T}_plain"] = _mlp(192, T, 2, B=2, i=1)
        c[f"mlp_res64_T{T}_tape"] = _mlp(64, T, 2, tape=True, env=MINC64, i=3)
        c[f"mlp_res64_T{T}_plain"] = _mlp(64, T, 0, env=MINC64)
        c[f"mlp_res96_T{T}_tape"] = _mlp(96, T, 1, tape=True, env=MINC64)           # K = 96: one and a half steps; fc2 K = 384
        c[f"mlp_res160_T{T}_plain"] = _mlp(160, T, 0, env=MINC64, i=1)              # K = 160: two and a half steps; fc2 K = 640
        c[f"mlp_res384_T{T}_smallm"] = _mlp(384, T, 0, tiled=True, i=1)             # small-M fc2, fp32 epilogue
        c[f"mlp_res192_T{T}_smallm"] = _mlp(192, T, 1, tiled=True, B=2, i=2)         # the same against the row loop's fc2 (K = 768); B = 2, HW odd
        # pick_cb just below its threshold: 18 units x 32 = 576 < 600 -> two blocks (T = 10: 143 = 11 x 13 positions; T = 20: 70 = 7 x 10)
        c[f"mlp_wide384_T{T}_cb2_below600"] = _mlp(384, T, 0, env=KRING, HW=(11, 13) if T == 10 else (7, 10))
    # C = 320 with Ch = 960 (Ch % 96 == 0): fc1 K = 320 = two and a half chunks of the ring; by default fc1 AND fc2 (K = 960 <= 1024) on the row loop
    c["mlp_wide320_T10"] = _mlp(320, 10, 0, 2, env=KRING, Ch=960)
    c["mlp_res320_T10_fc2_k960"] = _mlp(320, 10, 2, 1, Ch=960, i=1)
    # pm_ring_grid: fc1 with three blocks has 32 column groups; 34 units (T = 10, 17 x 16 = 272 positions) = 9 row groups: 288 items in
    # (256, 1024] -> 2 passes, 32 x 5 workgroups; 133 units (T = 20, 23 x 23 = 529 positions) = 34 row groups: 1 088 > 1 024 -> one pass again
    c["mlp_wide384_T10_passes2"] = _mlp(384, 10, 0, env=KRING, HW=(17, 16))
    c["mlp_wide384_T20_above1024"] = _mlp(384, 20, 0, env=KRING, HW=(23, 23), i=1)
    # res_row_ranges: fc1 at C = 192 has 24 column groups; 81 units (T = 20, 17 x 19 = 323 positions): 24 x ceil(81 / 8) = 264 > 256 -> two units per wave
    c["mlp_res192_T20_two_units_per_wave"] = _mlp(192, 20, 0, tape=True, HW=(17, 19))
    # ---- attention
    for cls in (0, 1, 2):
        e1, e2 = (cls + 1) % 3, (cls + 2) % 3
        st = "stacked" if cls != 1 else "separate"                # (every PSN has its own matrix: q and k are separate projections)
        # row loop, C = 192 (K = 192 small-K): front with and without the tape, the projection with epilogue 3 and 2
        c[f"attn_res192_T10_c{cls}_tape_emit{e1}"] = _attn(192, 10, cls, e1, tape=True, form=st, geom="w5s")
        c[f"attn_res192_T20_c{cls}_emit{e2}"] = _attn(192, 20, cls, e2, geom="w5")
        c[f"attn_res192_T20_c{cls}_tape"] = _attn(192, 20, cls, tape=True, geom="w5")
        # default routing at C = 384: the front and the projection (K = 384, not small-K) on the row loop
        c[f"attn_res384_T10_c{cls}_emit{e2}"] = _attn(384, 10, cls, e2, tape=cls == 0, form=st, geom="w9")
        c[f"attn_res384_T20_c{cls}_emit{e1}"] = _attn(384, 20, cls, e1, tape=cls == 1, geom="w5")
        # K ring, 16-token tiles (RB = 2)
        c[f"attn_wide384_T10_c{cls}_tape_emit{e2}"] = _attn(384, 10, cls, e2, tape=True, form=st, geom="w5s", env=KRING)
        c[f"attn_wide384_T20_c{cls}_emit{e1}"] = _attn(384, 20, cls, e1, geom="w5", env=KRING)
        # K ring, 32-token tiles (RB = 4): 2 500 rows, t5 x nH = 79 x 12 = 948 >= 800
        c[f"attn_wide384_T10_c{cls}_rb4_tape"] = _attn(384, 10, cls, tape=True, geom="w5big", env=KRING)
        c[f"attn_wide384_T10_c{cls}_rb4_emit{e1}"] = _attn(384, 10, cls, e1, form=st, geom="w5big", env=KRING)
    c["attn_res384_T10_plain"] = _attn(384, 10, 0, geom="w5s")                      # row loop, epilogue 2 at K = 384
    c["attn_res384_T20_plain"] = _attn(384, 20, 2, geom="w5")
    c["attn_res192_T10_plain"] = _attn(192, 10, 1, geom="w9")
    c["attn_wide384_T20_tape"] = _attn(384, 20, 1, tape=True, geom="w5", env=KRING)
    # K of the row loop: 64 (one step), 96 (one and a half), 160; K of the ring: 192 (one and a half chunks), 256, 320, 640 (odd: the single-chunk tail)
    for C, T, cls, em in ((64, 20, 1, 2), (96, 10, 0, 1), (160, 10, 2, 0)):
        c[f"attn_res{C}_T{T}"] = _attn(C, T, cls, em, tape=True, geom="w5s" if T == 10 else "w5", env=MINC64)
    for C, T, cls, em in ((192, 10, 0, 1), (256, 20, 1, 2), (320, 10, 2, 0), (640, 10, 1, 0)):
        c[f"attn_wide{C}_T{T}"] = _attn(C, T, cls, em, tape=C != 320, geom="w9" if C == 192 else "w5", env=KRING)
    # wide_front_kernel just below its rule: 1 000 rows at C = 768, t5 x nH = 32 x 24 = 768 < 800 -> still 16-token tiles
    c["attn_wide768_T10_rb2_below800"] = _attn(768, 10, 0, geom="w5mid", env=KRING)
    # res_row_ranges in the front: C = 512, 2 500 rows = 157 tiles: 16 heads x ceil(157 / 8) = 320 > 256 -> 16 tiles per range
    c["attn_res512_T10_two_tiles_per_wave"] = _attn(512, 10, 0, tape=True, geom="w5big")
    # ---- both families over the channel counts they share, 192 to 768 in steps of 64 (test_families: bit-equal): by default the row loop takes
    # fc1 and the projection (K = C <= 768) and, up to 512 channels, the front; under KRING the K ring takes them all
    for j, C in enumerate(range(192, 769, 64)):
        cls, T = j % 3, (10, 20)[j % 2]
        c[f"attn_fam{C}_T{T}"] = _attn(C, T, cls, (cls + 1) % 3, tape=j % 2 == 0, form="stacked" if cls == 0 else "separate", geom="w5")
        c[f"mlp_fam{C}_T{T}"] = _mlp(C, T, (cls + 1) % 3, cls, tape=j % 2 == 1, Ch=handover_Ch(C), i=j)
    # ---- patch merging: odd H and W; the row loop at C = 64 (K = 256: small-K), 96, 160, 256 (K = 1 024: the largest resident image); the ring at 320;
    # every strip-off build through SDF_RES_STRIP = 0
    for T in (10, 20):
        for C in (64, 96):
            c[f"merge_res{C}_T{T}"] = {"kind": "merge", "C": C, "D": T, "B": 2, "H": 5, "W": 7, "env": {}}
            c[f"merge_res{C}_T{T}_nostrip"] = {"kind": "merge", "C": C, "D": T, "B": 1, "H": 7, "W": 9, "env": dict(NOSTRIP)}
        c[f"merge_wide320_T{T}"] = {"kind": "merge", "C": 320, "D": T, "B": 1, "H": 5, "W": 7, "env": {}}
        # the transposed convolution: Cin = 64 (K = 256, small-K) and 96, Cout % 8 == 0 as the entry point asks (N = 4 Cout = 96 and 32 columns: 24 and 8 are no multiples of 16)
        for Cin, Cout in ((64, 24), (96, 8)):
            c[f"deconv{Cin}_T{T}"] = {"kind": "deconv", "imgs": T, "T": T, "H": 5, "W": 7, "Cin": Cin, "Cout": Cout, "env": {}}
            c[f"deconv{Cin}_T{T}_nostrip"] = {"kind": "deconv", "imgs": 2 * T, "T": T, "H": 3, "W": 5, "Cin": Cin, "Cout": Cout, "env": dict(NOSTRIP)}
    c["merge_res160_T10"] = {"kind": "merge", "C": 160, "D": 10, "B": 1, "H": 5, "W": 7, "env": {}}
    c["merge_res256_T10_k1024"] = {"kind": "merge", "C": 256, "D": 10, "B": 1, "H": 5, "W": 7, "env": {}}
    # ---- the plain product on row-major digits (T = 10 by construction): K = 128, 256 (the last small-K build), 288 (the first other one
    # an entry point admits: res_pm_takes would take K = 272 - K % 16 == 0 but not % 32, valid only without the scramble map - but
    # sdf_spike_gemm_fwd asks K % 32 == 0 of every product, the merge has K = 4 C with C % 32 == 0 and the transposed convolution K = 4 Cin
    # with Cin % 16 == 0: no call reaches the row loop with K % 32 != 0, test_k272_is_refused holds the entry point to that), 1 024;
    # M = 350: 35 "positions"
    for K in (128, 256, 288, 1024):
        c[f"gemm_k{K}"] = {"kind": "gemm", "M": 350, "N": 96, "K": K, "env": {}}
    for K in (128, 288):
        c[f"gemm_k{K}_nostrip"] = {"kind": "gemm", "M": 350, "N": 96, "K": K, "env": dict(NOSTRIP)}
    return c


CASES = _cases()


def shape_of(s):
    """(positions of the stream, rows of the attention or None) of an MLP / attention case"""
    if s["kind"] == "mlp":
        return s["B"] * s["H"] * s["W"], None
    B, H, W, window, _ = GEOM[s["geom"]]
    nwin = B * cdiv(s["D"], window[0]) * cdiv(H, window[1]) * cdiv(W, window[2])
    return B * H * W, nwin * window[1] * window[2]


def route(s, env=None):
    """the launch lines of a case under its own switches (or under `env`)"""
    env = s["env"] if env is None else env
    k = s["kind"]
    if k == "mlp":
        return route_mlp(s["C"], s["Ch"], s["D"], shape_of(s)[0], s["cls"], s["emit"], s["tape"], s["tiled"], env)
    if k == "attn":
        pos, rows = shape_of(s)
        return route_attn(s["C"], s["D"], pos, rows, s["cls"], s["emit"], s["tape"], env)
    if k == "merge":
        return route_merge(s["C"], 2 * s["C"], s["D"], s["B"] * cdiv(s["H"], 2) * cdiv(s["W"], 2), env)
    if k == "gemm":
        return route_gemm(s["M"], s["N"], s["K"], env)
    return route_deconv(s["imgs"], s["T"], s["H"], s["W"], s["Cin"], s["Cout"], env)


def other_family(s):
    """The switches under which ANOTHER kernel family serves the same call (the same integer sums, the same fp32 epilogue expressions:
    every output bit-equal), or None: the K ring for a row-loop case of C % 64 == 0 from 192 channels on (the merge: SDF_RES=0 from 64
    on), for fc2 on the small-M kernel the main loop that takes it with the small-M kernel off: the K ring at C = 384 (K = 1 536), the row
    loop at C = 192 (K = 768)."""
    k, env = s["kind"], s["env"]
    if k == "mlp" and s["tiled"]:
        return {**env, "SDF_SMALLM_FC2": "0"}
    if k in ("mlp", "attn") and not env and s["C"] >= 192 and s["C"] % 64 == 0 and (k == "attn" or s["Ch"] % 96 == 0):
        return dict(KRING)
    if k == "merge" and s["C"] % 64 == 0 and s["C"] <= 256 and not env:
        return {"SDF_RES": "0"}
    return None


def kernels(lines):
    return {line.split(" ", 3)[3] for line in lines}
