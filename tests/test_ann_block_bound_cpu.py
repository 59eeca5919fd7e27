"""The per-element bound of the ANN half blocks' parity tests (tests/ann_block_cases.py), fixed WITHOUT a kernel: attainable by the
numerics the kernels document, and sharp enough to see one missing cross term of a three-product fp16 split.

For every case: r32 (ann_block_cases.R32, recomputed here) = max |branch32 - branch64| / B (the fp64 reference against the same reference in plain fp32, per element over the
magnitude sum B of the last product) and tol = 8 r32 - 4 for the two bits by which hi hi + hi lo + lo hi (22 bits) falls short of an fp32
product (24), 2 for the dropped lo lo term and the hardware's v_exp_f32 / v_rcp_f32 at 1 ulp, which libm does not share.  Nothing here
is fitted to what a kernel returns.  Then, with ratio = max |(out - x) - branch64| / (tol B + 2^-23 |x + branch64| (+ GELU term)):

  * the emulation of the documented numerics (ann_block_cases.attn_emulate / mlp_emulate) stays below 1 on every case - as it stands,
    WITHOUT any allowance for the fp16 subnormal floor of the lo planes (2^-25 absolute per weight; every weight of both recipes has
    a subnormal lo half): the worst case uses 0.61 of the allowance;
  * with one cross term dropped from ANY product the ratio is above 1 on every plain "ls10" case of both recipes - asserted for the
    last product (proj, fc2) as the bound's reason for being, and for qkv, K Q^T, P V and fc1 as well since they all exceed it too;
  * a matrix pipe that flushed fp16 subnormal inputs (ftz) is above 1 on every plain "ls10" case: whether gfx950 does is then decided
    by test_ann_block_parity_gpu.py passing.
On the "ls100", "mean50" cases the fp32 rounding of the logits (up to 116) or of the centred input dominates r32, tol is ten times
looser and a dropped term of P V stays as low as 1.7 x: those cases are kept for their code paths, not for sharpness.

Measured (`a.b`: term b of product a dropped; hl = a_hi b_lo, lh = a_lo b_hi in mma3's operand order):

  attention case                 r32      tol      full proj.hl proj.lh   pv.hl   pv.lh   qk.hl   qk.lh  qkv.hl  qkv.lh     ftz
  flat1-wide-ls10                1.38e-07 1.10e-06 0.17    39.0    46.4    20.1    31.5    62.1    55.0    75.7    78.0   106.3
  flat1-init-ls10                1.21e-07 9.66e-07 0.41    35.6    36.0    22.7    23.2    40.0    57.9    73.2    67.2    94.3
  flat8-wide-ls10                1.47e-07 1.17e-06 0.18    45.2    44.6    23.7    32.7    60.9    60.2   131.6    93.7   117.5
  flat8-init-ls100               1.82e-06 1.45e-05 0.61     7.9     6.5     3.1     6.8    67.6    84.8    81.3   119.5   145.6
  flat12-init-ls10               1.80e-07 1.44e-06 0.35    31.7    28.4    14.5    24.9    43.9    70.0    61.0    67.4    75.3
  flat12-wide-ls100              2.16e-06 1.73e-05 0.14     5.0     5.1     2.2     4.9    50.0    65.7    83.9   126.2   125.8
  flat17-wide-ls10               1.83e-07 1.46e-06 0.15    40.5    42.1    18.8    37.4    52.2    71.5    89.9    75.4   103.6
  flat17-init-ls10               1.88e-07 1.50e-06 0.36    27.7    33.6    16.6    27.0    48.7    53.7    67.6    61.0    89.5
  mask4-wide-ls10                1.86e-07 1.49e-06 0.17    45.7    46.2    21.4    41.0    88.6    78.5   139.6   125.1   152.2
  mask4-init-ls10                2.08e-07 1.67e-06 0.46    39.4    44.4    21.7    36.6    61.2    59.7    76.7    95.7   123.9
  mask4-wide-ls100               1.40e-06 1.12e-05 0.16     8.7    11.2     4.0     9.2    75.4    96.5   129.9   116.2   104.9
  mask12-wide-ls10               2.14e-07 1.71e-06 0.16    48.1    45.2    22.9    38.4    56.0    72.7    98.9   106.2   124.8
  mask12-init-ls10               2.28e-07 1.82e-06 0.42    35.6    31.9    19.2    35.5    54.4    53.6    69.1    74.5   112.6
  mask12-init-ls100              2.04e-06 1.63e-05 0.48     6.5     7.8     3.5     7.0    60.3    69.1   105.3   112.5   146.4
  pad-wide-ls10                  2.48e-07 1.98e-06 0.18    35.6    37.4    30.6    31.7    67.9    81.3    89.1    95.6   104.8
  pad-init-ls10                  3.46e-07 2.77e-06 0.29    21.8    24.3    11.1    23.3    50.7    39.2    52.8    64.3   103.5
  padshift-wide-ls10             2.34e-07 1.87e-06 0.14    38.4    41.0    19.4    32.3    45.9    78.8    94.7    79.0    82.7
  padshift-init-ls10             2.33e-07 1.87e-06 0.41    30.3    38.9    15.9    30.8    37.9    53.7    61.0    92.0   106.0
  padshift-wide-ls100            1.96e-06 1.57e-05 0.25     6.3     7.0     2.9     6.6    58.2    74.5    96.8   103.6   111.1
  mask4-wide-ls10-noqkvbias      1.82e-07 1.46e-06 0.16    47.3    48.3    23.4    48.8    74.0    70.0    98.4    96.0   119.3
  padshift-init-ls10-noprojbias  1.96e-07 1.57e-06 0.43    44.4    44.3    21.9    43.6    55.1    77.0   100.2   100.0   150.3
  mask4-init-ls10-smallx         1.96e-07 1.57e-06 0.49    45.2    43.7    22.0    38.9    61.8    66.6   100.2    86.2   148.2
  flat8-wide-ls10-mean50         1.68e-06 1.34e-05 0.19     4.1     3.7     1.7     3.3     5.3     6.9     7.8     8.6    10.0

  MLP case                       r32      tol      full  fc2.hl  fc2.lh  fc1.hl  fc1.lh     ftz
  r1-wide                        5.70e-08 4.56e-07 0.13    62.1    62.9    86.1    66.9    92.1
  r1-init                        6.64e-08 5.32e-07 0.26    44.2    38.2    37.3    56.2    78.4
  r15-wide                       2.24e-07 1.80e-06 0.09    32.3    32.3    34.5    34.5    48.0
  r15-init                       1.46e-07 1.17e-06 0.23    30.5    33.2    41.5    34.4    58.4
  r16-wide                       1.34e-07 1.07e-06 0.11    40.4    51.6    48.7    53.4    77.7
  r16-init                       1.12e-07 8.98e-07 0.37    44.2    42.0    40.6    46.4    79.7
  r17-wide                       1.38e-07 1.11e-06 0.11    47.1    46.3    51.1    50.5    70.3
  r17-init                       1.23e-07 9.83e-07 0.33    44.4    38.1    45.0    39.2    67.6
  r191-wide                      2.66e-07 2.13e-06 0.09    30.5    32.1    38.3    34.1    46.9
  r191-init                      2.89e-07 2.31e-06 0.16    24.4    25.5    22.4    25.5    43.0
  r192-wide                      2.55e-07 2.04e-06 0.09    33.5    35.3    43.4    35.4    51.6
  r192-init                      2.93e-07 2.34e-06 0.19    22.8    26.0    24.7    26.5    46.1
  r193-wide                      2.77e-07 2.21e-06 0.09    31.5    37.1    39.8    35.8    49.7
  r193-init                      2.40e-07 1.92e-06 0.20    30.3    27.9    33.0    33.0    51.5
  r385-wide                      2.95e-07 2.36e-06 0.10    31.9    36.6    34.4    33.9    46.3
  r385-init                      3.04e-07 2.44e-06 0.18    25.9    24.1    22.7    24.6    47.5
  r193-wide-nob1                 3.28e-07 2.63e-06 0.06    32.5    32.3    27.5    30.8    36.8
  r193-init-nob2                 2.00e-07 1.60e-06 0.23    34.2    34.3    32.3    37.8    66.9
  r193-wide-reach                3.92e-07 3.14e-06 0.06    23.4    24.4    27.8    34.7    39.2
  r193-init-reach                3.93e-07 3.14e-06 0.17    27.5    26.0    28.9    25.5    45.7
"""
import pytest

import ann_block_cases as AC

TERMS = ("hi_lo", "lo_hi")
# r32 is the maximum of a rounding error over the elements: it moves with the order in which the BLAS of the day sums (0.4 x to 2.0 x
# between 1 and 16 threads on the cases with few rows).  The recorded values stand; this window only says they are this reference's.
R32_WINDOW = 3.0
PRODUCTS = {"attn": ("proj", "pv", "qk", "qkv"), "mlp": ("fc2", "fc1")}


def measure(name, kind, products=None, ftz=True):
    """{"r32", "tol", "full", "<product>.<term>"..., "ftz"}: r32 and the worst ratio of the emulation, whole, with each cross term
    of each product dropped, and on a pipe that flushes subnormals."""
    case, emulate = (AC.attn_case(name), AC.attn_emulate) if kind == "attn" else (AC.mlp_case(name), AC.mlp_emulate)
    r, tol = AC.r32(name, kind), AC.tol(name)
    out = {"r32": r, "tol": tol, "full": AC.worst_ratio(emulate(case), name, kind, tol)}
    for p in PRODUCTS[kind] if products is None else products:
        for t in TERMS:
            out[f"{p}.{t}"] = AC.worst_ratio(emulate(case, (p, t)), name, kind, tol)
    if ftz:
        out["ftz"] = AC.worst_ratio(emulate(case, ftz=True), name, kind, tol)
    return out


def _row(name, m):
    return f"{name:30s} {m['r32']:.2e} {m['tol']:.2e} {m['full']:.2f} " + " ".join(f"{v:7.1f}" for k, v in m.items() if "." in k or k == "ftz")


@pytest.mark.parametrize("name", list(AC.ATTN_CASES))
def test_attention_bound_is_attainable_and_sharp(name):
    sharp = name in AC.SHARP
    m = measure(name, "attn", None if sharp else (), ftz=sharp)
    print("\nANNBOUND attn " + _row(name, m))
    assert AC.R32[name] / R32_WINDOW <= m["r32"] <= AC.R32[name] * R32_WINDOW, "the recorded r32 is not this reference's fp32 error"
    assert m["full"] < 1.0
    for k, v in m.items():
        if "." in k or k == "ftz":
            assert v > 1.0, (k, v)


@pytest.mark.parametrize("name", list(AC.MLP_CASES))
def test_mlp_bound_is_attainable_and_sharp(name):
    sharp = name in AC.SHARP_MLP
    m = measure(name, "mlp", None if sharp else (), ftz=sharp)
    print("\nANNBOUND mlp " + _row(name, m))
    assert AC.R32[name] / R32_WINDOW <= m["r32"] <= AC.R32[name] * R32_WINDOW, "the recorded r32 is not this reference's fp32 error"
    assert m["full"] < 1.0
    for k, v in m.items():
        if "." in k or k == "ftz":
            assert v > 1.0, (k, v)
    if "reach" in name:
        hpre = AC.mlp_ref(name)["hpre"]
        assert hpre.min().item() < -5.0 and hpre.max().item() > 5.0           # both tails of the GELU polynomial are entered


def test_row_map_is_the_oracles_slice_table():
    """row_map_cpu (pad / roll / partition on row indices) equals the oracle's closed-form slice table, itself pinned to the reference;
    padding tokens sit inside windows (not only at their ends) in the padded geometries."""
    import torch
    from oracle import sdformer_oracle as O
    for g, (B, D, H, W, ss) in AC.GEOMETRY.items():
        m, B_, _ = AC.row_map_cpu(B, D, H, W, ss)
        src, B2 = O.slice_table(B, D, H, W, AC.WS, ss)
        assert B_ == B2 and torch.equal(m.long(), torch.from_numpy(src).reshape(-1)), g
        valid = m[m >= 0].long()
        assert torch.equal(valid.sort().values, torch.arange(B * D * H * W)), g     # every row belongs to exactly one window token
        if g.startswith("pad"):
            w16 = (m.view(B_, AC.N)[:, :160].reshape(B_, 10, 16) < 0).sum(-1)
            assert bool(((w16 > 0) & (w16 < 16)).any()), g                         # a wave's 16 tokens: some padding, some not
