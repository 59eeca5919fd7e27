"""The one-launch ANN half blocks (csrc/ann_block.hip: LayerNorm -> qkv -> cosine window attention -> proj -> + x; csrc/ann_mlp_block.hip:
LayerNorm -> fc1 -> GELU -> fc2 -> + x) called directly - hip.ann_attn_block / hip.ann_mlp_block with the packers, no module - and held,
per element, to the float64 branch of tests/ann_block_cases.py:

  |(out - x) - branch64| <= tol B + 2^-23 |x + branch64| (+ 1.5e-7 sum_j |W2[c,j]| |hpre[t,j]| for the MLP's polynomial erf),

B the magnitude sum of the last product, tol = 8 x the reference's own fp32 error over B (ann_block_cases.R32, derived and shown
attainable and sharp by test_ann_block_bound_cpu.py without a kernel: one missing hi lo or lo hi term of proj / fc2 exceeds it 20 to
60 times on the "ls10" cases).  The shortcut x, ten times the branch, is no part of the scale.  Every case also

  * asserts through hip.launch_log() that exactly ONE launch happened, of ann_attn_block_kernel / ann_mlp_block_kernel, 768 threads, the
    file's LDS_BYTES, B_ / ceil(rows / 192) workgroups - a parity test that silently ran the 4 + 3 launch path proves nothing;
  * hands the kernel an `out` that is a slice of a larger buffer, 64 guard rows on each side, everything NaN beforehand: the guards hold
    the same NaN bits afterwards, no NaN remains inside (both kernels store through 2^31 - 1 byte buffer descriptors: nothing clamps a
    wrong row), and the input is unchanged;
  * runs twice: bit-equal.
In place (`out is x`) both kernels return the bits of the out-of-place call - for attention on the shifted, padded map, where the
rows of a window are spread over the map and other windows' rows are in flight.

What the cases are for: ann_block_cases.GEOMETRY / ATTN_CASES / MLP_CASES.

Measured on an MI355X, worst err / allowance per kernel, recipe and logit scale (tol: the CPU-derived 8 r32 of the worst case; the
emulation's own worst figure on the CPU, for comparison, is 0.61):
  attention  wide ls10  0.23 (tol 1.5e-6)   wide ls100 0.19 (tol 1.1e-5)   init ls10 0.52 (tol 1.6e-6)   init ls100 0.55 (tol 1.5e-5)
  MLP        wide       0.16 (tol 1.1e-6)   init       0.29 (tol 9.8e-7)
fp16 subnormals: MEASURED, gfx950's v_mfma_f32_16x16x32_f16 (and the 32x32x16 of dense_linear.hip) consumes subnormal fp16 inputs
without flushing them.  Every lo plane of every weight here is subnormal (|w| < 0.25), and a pipe that flushed them would sit at 40 to
150 times the allowance on every case (test_ann_block_bound_cpu.py, column ftz); the kernels sit where the un-flushed emulation does.
Once, with a diagnostic library whose mma3 lacked its a_lo b_hi product: all 43 parity cases failed, at 10 (mean50) and 35 to 162
times the allowance - the figures the CPU emulation predicts for that fault.
Run time there: the 47 cases of this file and the 25 of test_dense_linear_gpu.py in 3.2 s together; the first (it loads the library)
0.7 s, every other 0.01 s.
"""
import functools
import math

import pytest
import torch

import ann_block_cases as AC
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                       # guard rows on each side of `out`


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


def _guarded(rows):
    buf = torch.full((GUARD + rows + GUARD, AC.C), float("nan"), device=DEV)
    bits = buf.view(torch.int32)
    return buf, bits, int(bits[0, 0])


def _launch(call, x, inplace):
    """One call into a NaN-filled, guarded `out` (in place: `out` holds x and is the input too) -> (result on the CPU, launch log)."""
    rows = x.shape[0]
    buf, bits, nan_bits = _guarded(rows)
    out = buf[GUARD:GUARD + rows]
    xg = _dev(x)
    if inplace:
        out.copy_(xg)
        xg = out
    with hip.launch_log() as log:
        call(xg, out)
    torch.cuda.synchronize()
    assert bool((bits[:GUARD] == nan_bits).all()) and bool((bits[GUARD + rows:] == nan_bits).all()), "a store outside `out`"
    got = out.cpu()
    assert not torch.isnan(got).any(), "an output row was never written"
    if not inplace:
        assert torch.equal(xg.cpu(), x), "the input was written"
    return got, log


def _assert_one_launch(log, kernel, wgs, lds):
    assert len(log.rows) == 1, log.rows
    name, n, threads, lds_bytes, _ = log.rows[0]
    assert kernel in name, name
    assert (n, threads, lds_bytes) == (wgs, 768, lds), log.rows[0]


@functools.lru_cache(maxsize=None)
def _attn_args(name):
    """Device arguments of one attention case, made as the module makes them: the slice map on the device, the fp16 planes and the
    (bias + mask) * log2 e table from the packers."""
    c = AC.attn_case(name)
    B, D, H, W, ss = c.geom
    row_map, B_ = hip.window_slice_map(B, D, H, W, AC.WS, ss, DEV)
    assert B_ == c.B_ and torch.equal(row_map.cpu(), c.row_map), "the device's slice map is not pad / roll / partition"
    wq, wp = hip.pack_ann_attn_block_weights(_dev(c.wqkv), _dev(c.wproj), AC.NH)
    scale = torch.clamp(_dev(c.ls), max=math.log(1.0 / 0.01)).exp().reshape(-1).contiguous()      # WindowAttention3D._bias_and_scale
    scale2, table = hip.ann_attn_block_table(scale, _dev(c.bias), _dev(c.mask))
    assert table.shape[0] == (1 if c.mask is None else c.mask.shape[0]) and c.B_ % table.shape[0] == 0
    return row_map, wq, wp, scale2, table, _dev(c.ln_w), _dev(c.ln_b), _dev(c.bqkv), _dev(c.bproj)


def _run_attn(name, inplace=False):
    c = AC.attn_case(name)
    row_map, wq, wp, scale2, table, ln_w, ln_b, bqkv, bproj = _attn_args(name)
    call = lambda x, out: hip.ann_attn_block(x, out, row_map, c.B_, AC.N, AC.NH, ln_w, ln_b, AC.EPS, wq, bqkv, scale2, table, wp, bproj)
    got, log = _launch(call, c.x, inplace)
    _assert_one_launch(log, "ann_attn_block_kernel", c.B_, AC.ATTN_LDS)
    return got


@functools.lru_cache(maxsize=None)
def _mlp_args(name):
    c = AC.mlp_case(name)
    w1, w2 = hip.pack_ann_mlp_block_weights(_dev(c.w1), _dev(c.w2))
    return w1, w2, _dev(c.ln_w), _dev(c.ln_b), _dev(c.b1), _dev(c.b2)


def _run_mlp(name, inplace=False):
    c = AC.mlp_case(name)
    w1, w2, ln_w, ln_b, b1, b2 = _mlp_args(name)
    call = lambda x, out: hip.ann_mlp_block(x, out, ln_w, ln_b, AC.EPS, w1, b1, w2, b2)
    got, log = _launch(call, c.x, inplace)
    _assert_one_launch(log, "ann_mlp_block_kernel", -(-c.x.shape[0] // AC.ROWS_WG), AC.MLP_LDS)
    return got


def _check(run, name, kind):
    got = run(name)
    ratio = AC.worst_ratio(got, name, kind, AC.tol(name, kind))
    print(f"\nANNPARITY {kind} {name} err/allowance {ratio:.3f} tol {AC.tol(name, kind):.2e}")
    assert ratio <= 1.0, ratio
    assert torch.equal(run(name), got), "two calls differ"


@pytest.mark.parametrize("name", list(AC.ATTN_CASES))
def test_attention_half_block_per_element(name):
    assert hip.ann_attn_block_supported(AC.C, AC.NH, AC.N)
    _check(_run_attn, name, "attn")


@pytest.mark.parametrize("name", list(AC.MLP_CASES))
def test_mlp_half_block_per_element(name):
    assert hip.ann_mlp_block_supported(AC.C, AC.CH)
    _check(_run_mlp, name, "mlp")


@pytest.mark.parametrize("name", ["padshift-wide-ls10", "padshift-init-ls10-noprojbias"])
def test_attention_half_block_in_place(name):
    """out is x on the shifted, padded map: a workgroup reads its window's rows at the start and again for the shortcut at the end,
    while the workgroups of other windows write theirs - every row belongs to one window, so the bits are those of the
    out-of-place call."""
    assert torch.equal(_run_attn(name, inplace=True), _run_attn(name))


@pytest.mark.parametrize("name", ["r193-wide", "r385-init"])
def test_mlp_half_block_in_place(name):
    assert torch.equal(_run_mlp(name, inplace=True), _run_mlp(name))
