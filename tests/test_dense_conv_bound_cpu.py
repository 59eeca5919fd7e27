"""The per-element bound of the dense convolution's parity test (tests/dense_conv_cases.py), settled WITHOUT a kernel: attainable by
the arithmetic the kernel documents, sharp enough to see the faults a convolution kernel of this kind can have, and a case set that
- by the launcher's dispatch restated on the CPU - reaches every instantiation on both grids.

TOL = 2e-6 (the per-element constant of test_dense_linear_gpu.py) stands: the emulation's worst (|err| - fmt) / mag over the random
cases is 4.1e-7, 8 x that is 3.3e-6 - no tighter constant to take.  With ratio = max |out - ref64| / (TOL mag + fmt), measured here
(columns: the honest emulation; a_lo w_hi missing; w_lo a_hi missing; fp16 subnormal halves flushed to zero; the centre tap dropped at
one border pixel; the residual read from the next column block):

  case                  full  -alo.whi  -wlo.ahi      ftz      tap  resid_cb
  tiny-3x5x9-c16        0.50      81.3      91.4      529  1.0e+05         -
  tiny-2x4x8-c16        0.04      62.4      62.6      2.3  8.9e+04         -
  tiny-1x7x17-c16       0.32      83.7      82.6      108  9.5e+04         -
  tiny-5x3x31-c16       0.49      81.6      91.6     1258  9.3e+04         -
  tiny-3x5x9-c96        0.49      42.7      45.8      141  2.8e+04         -
  tiny-2x4x8-c96        0.09      29.2      42.8     28.6  5.6e+04         -
  tiny-1x7x17-c96       0.49      44.0      39.9      944  4.0e+04         -
  tiny-5x3x31-c96       0.49      37.9      41.8     1445  1.0e+05         -
  p11-none              0.49      81.9     109.1      212  8.8e+04         -
  p11-cin10-all         0.10     157.8     120.1      199  1.1e+05   9.4e+07
  p11-wider             0.24      80.1     100.2      379  1.1e+05         -
  p61-none              0.49      53.2      47.0     1570  5.8e+04         -
  p61-ab                0.24      54.7      37.2      429  3.6e+04         -
  p61-res               0.42      46.4      55.2      333  4.6e+04   3.9e+07
  p61-relu              0.48      35.9      53.6     1185  2.5e+04         -
  p61-f32               0.06      52.6      52.3  1.6e+04  4.6e+04         -
  p61-all               0.10      37.3      39.2      234  4.5e+04   2.4e+07
  p61-all-f32           0.07      40.5      46.1     80.3  4.2e+04   1.1e+08
  p61-narrow            0.07      35.9      30.5      123  3.2e+04         -
  p61-wider             0.37      51.0      41.2      268  6.0e+04         -
  p62-all               0.06      38.1      39.0     64.9  3.0e+04         -
  p62-f32               0.11      59.1      50.8  2.6e+04  5.6e+04         -
  p62-edges             0.24      57.8      48.8      497  8.3e+04         -
  p62-forced61          0.07      37.7      42.9     64.5  4.4e+04         -
  p61-forced62          0.16      34.9      29.3     69.7  3.0e+04   2.3e+07
  f61-n96               0.42      63.5      65.0      499  5.5e+04   4.3e+07
  f62-n192              0.12      62.8      75.5     3456  6.5e+04         -
  f11-n64               0.41     136.0     120.0      822  1.1e+05   5.6e+07
  f11-walk              0.17     140.8     159.0  1.2e+05  1.0e+05         -
  chain-7               0.37      50.6      35.1      709  4.2e+04         -
  chain-13              0.41      36.6      30.0      309  2.6e+04         -
  deconv-96-18          0.50      42.8      50.0      747  1.5e+05         -

The honest emulation's worst ratio is 0.50 (the plane store's 2^-22 against fmt = 2^-21; 0.17 where the output is fp32); the
smallest figure of any fault is 2.3 (ftz on a map of 64 pixels), of a missing cross product 29.  The four maps of fewer than 64
pixels (tiny-1x1x1, tiny-1x2x3) lie in one or two blocks of the activation scale: the emulation stays inside there too (0.40 - 0.49)
and the dropped tap shows (5.5 to 7.6e4), but a map whose one scale is 1e-6 has no lo half to lose, so the product and ftz faults
are asserted from 64 pixels on.  The figures include the allowance's floor for fp16-subnormal halves (dense_conv_cases' docstring):
without it the ftz column of the fp32 cases is 4 to 6 times larger and nothing else moves by more than 3 %.
"""
import pytest
import torch

import dense_conv_cases as DC

FAULTS = ("no_alo_whi", "no_wlo_ahi", "ftz", "tap", "resid_cb")
E_WINDOW = 3.0                                   # E_EMU is a maximum of rounding errors: it moves with the BLAS's summation order


def _pixels(name):
    s = DC.SHAPES[name]
    return s.imgs * s.H * s.W


def _fmt(v):
    return f"{v:9.2f}" if v < 100 else (f"{v:9.0f}" if v < 1e4 else f"{v:9.1e}")


@pytest.mark.parametrize("name", list(DC.SHAPES))
def test_exact_cases_are_exact(name):
    """The operands keep their promises (dense_conv_cases.assert_exact) and the emulation of the kernel's arithmetic - three fp16
    products, fp32 sums, fp32 epilogue, the plane store - returns the fp64 result bit for bit."""
    bits = DC.assert_exact(name)
    out = DC.emulate(name, "exact")
    assert torch.equal(out.double(), DC.reference(name, "exact")["ref"])
    print(f"\nDENSEEXACT {name} magnitude / unit: {bits:.1f} bits")


@pytest.mark.parametrize("name", list(DC.SHAPES))
def test_bound_is_attainable_and_sharp(name):
    s = DC.SHAPES[name]
    full = DC.ratio(DC.emulate(name, "random"), name, "random").max().item()
    row = {}
    for f in FAULTS:
        if f == "resid_cb" and not (s.resid and s.N >= 64):
            continue
        if f in ("no_alo_whi", "no_wlo_ahi", "ftz") and _pixels(name) < 64:
            continue
        row[f] = DC.ratio(DC.emulate(name, "random", f), name, "random").max().item()
    print(f"\nDENSEBOUND {name:18s} {full:6.2f} " + " ".join(_fmt(row[f]) if f in row else "        -" for f in FAULTS))
    assert full < 1.0
    for f, v in row.items():
        assert v > 1.0, (f, v)


def test_tolerance_is_the_projects_and_the_emulation_shows_no_tighter_one():
    worst = max(DC.err_over_mag(DC.emulate(n, "random"), n, "random") for n in DC.SHAPES)
    print(f"\nDENSEBOUND worst (|err| - fmt) / mag of the emulation {worst:.2e}; recorded {DC.E_EMU:.2e}; TOL {DC.TOL:.1e}")
    assert DC.E_EMU / E_WINDOW <= worst <= DC.E_EMU * E_WINDOW, "the recorded E_EMU is not this emulation's"
    assert DC.TOL == 2e-6 and worst < DC.TOL


def test_random_cases_have_what_the_bound_is_for():
    """Whole windows with fp16-subnormal hi halves, a silent image, a dead column, negative alphas."""
    for name in ("p61-all", "f61-n96", "f11-n64"):
        o = DC.operands(name, "random")
        own = o.x.abs().amax(1)
        assert bool((own[own > 0] < 2.0 ** -14).any())
        assert o.zero_img is not None and torch.count_nonzero(o.x[o.zero_img]) == 0
        assert o.alpha[o.zero_col] == 0 and o.beta[o.zero_col] == 0 and bool((o.alpha < 0).any())
        assert float(own.max() / own[own > 0].min()) > 1e6                        # the pixels' scales span 1e-7 .. 1e2


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def test_workgroup_map_serves_every_range_and_column_block_once():
    for name in DC.SHAPES:
        for r in DC.routes(name):
            served = sorted((rng, cb) for rng, cb, br in DC.workgroups(r) if br != "surplus")
            assert served == [(rng, cb) for rng in range(r.ranges) for cb in range(r.ncb)], name
            assert r.G == (256 if r.full else r.ranges * r.ncb)


def test_walk_multiplies_every_tile_once():
    for name, s in DC.SHAPES.items():
        for r in DC.routes(name):
            w = DC.walk(r, s.H, s.W)
            tiles_x, tiles_y = DC.cdiv(s.W, DC.TW), DC.cdiv(s.H, r.TH)
            assert sorted(w["tiles"]) == [(i, y, x) for i in range(s.imgs) for y in range(tiles_y) for x in range(tiles_x)], name


def test_cases_reach_every_instantiation_on_both_grids():
    seen = {(r.kernel, r.full) for n in DC.SHAPES for r in DC.routes(n)}
    assert seen == {(k, f) for k in ("<1, 1>", "<6, 1>", "<6, 2>") for f in (False, True)}
    fulls = {n: DC.routes(n)[0] for n in DC.SHAPES if DC.routes(n)[0].full}
    assert {r.kernel for r in fulls.values()} == {"<1, 1>", "<6, 1>", "<6, 2>"}
    for n, r in fulls.items():
        assert r.wtiles % r.ranges != 0, n                                       # rem != 0: ranges of two lengths
    count = lambda r, b: sum(1 for _, _, br in DC.workgroups(r) if br == b)
    r = fulls["f61-n96"]
    assert (r.ncb, r.ranges, r.wtiles) == (3, 85, 1026) and count(r, "pooled") == 15 and count(r, "surplus") == 1
    r = fulls["f62-n192"]
    assert (r.ncb, r.ranges, r.wtiles) == (6, 42, 342) and count(r, "pooled") == 12 and count(r, "surplus") == 4
    for n in ("f11-n64", "f11-walk"):                                            # ncb divides 32: whole groups only
        assert count(fulls[n], "pooled") == 0 and count(fulls[n], "surplus") == 0 and count(fulls[n], "whole") == 256
    assert fulls["f11-n64"].ranges == 128 and fulls["f11-walk"].ranges == 32
    # forced through SDF_DENSE_TPW on a shape whose rule picks the other
    for n, forced in (("p62-forced61", "<6, 1>"), ("p61-forced62", "<6, 2>")):
        s = DC.SHAPES[n]
        assert DC.routes(n)[0].kernel == forced != DC.dispatch(s.imgs, s.H, s.W, 6, s.N).kernel
    # and by the rule alone
    assert DC.routes("p61-none")[0].kernel == "<6, 1>" and DC.routes("p62-all")[0].kernel == "<6, 2>" and DC.routes("p11-none")[0].kernel == "<1, 1>"
    assert [r.kernel for r in DC.routes("chain-7")] == ["<6, 1>", "<1, 1>"]
    assert [r.kernel for r in DC.routes("chain-13")] == ["<6, 2>", "<6, 2>", "<1, 1>"]
    assert [r.cch for r in DC.routes("deconv-96-18")] == [6, 6] and DC.records_of(DC.SHAPES["deconv-96-18"])[0] == 12


def test_cases_reach_the_loaders_and_the_walks_edges():
    def prop(name):
        s, r = DC.SHAPES[name], DC.routes(name)[0]
        w = DC.walk(r, s.H, s.W)
        return s, r, w, [DC.interior(r, s.H, s.W, ty, tx) for _, ty, tx in w["tiles"]]
    # the interior-tile loader, for one and for two pixel blocks per wave; maps made of edge tiles only
    for name in ("p61-none", "p62-all", "f61-n96"):
        s, r, w, inner = prop(name)
        assert DC.interior(r, s.H, s.W, 1, 1) and any(inner) and not all(inner), name
    for name in ("p62-edges", "f62-n192", "f11-walk", "p61-narrow", "tiny-1x1x1-c16", "tiny-5x3x31-c96"):
        assert not any(prop(name)[3]), name
    # waves without a tile
    for name in ("p62-all", "tiny-5x3x31-c16", "tiny-1x1x1-c96"):
        assert 0 in prop(name)[2]["items"], name
    # odd step counts (one record only): 1, and 3 behind a whole pipelined pair
    assert set(prop("tiny-3x5x9-c16")[2]["items"]) == {1}
    s, r, w, _ = prop("f11-walk")
    assert set(w["items"]) == {2, 3} and DC.cdiv(s.W, DC.TW) == 1 < r.NW and DC.cdiv(s.H, r.TH) == 2      # a step of 12 tiles = 6 images
    assert (r.wtiles // r.ranges) % 2 == 1                                       # ranges begin in the middle of an image
    # several tiles per wave for six records too: wave 0 of the ranges that hold NW + 1
    for name in ("f61-n96", "f62-n192"):
        assert set(prop(name)[2]["items"]) == {1, 2}, name
    s, r, w, _ = prop("p61-narrow")
    assert DC.cdiv(s.W, DC.TW) == 1 and s.imgs == 5 and r.ranges == 2
    # sizes that are no multiple of the tile; the maps of tools/probes/dense_tiny_shapes.py
    assert any(s.H % 4 and s.W % 8 for s in DC.SHAPES.values())
    for imgs, H, W in ((1, 1, 1), (1, 2, 3), (3, 5, 9), (2, 4, 8), (1, 7, 17), (5, 3, 31)):
        for Cin, N in ((16, 32), (96, 64)):
            s = DC.SHAPES[f"tiny-{imgs}x{H}x{W}-c{Cin}"]
            assert (s.imgs, s.Cin, s.N, s.H, s.W) == (imgs, Cin, N, H, W)
    # epilogues: none, alpha / beta, residual, ReLU, fp32 against planes, all together
    epi = {(s.affine, s.resid, s.relu, s.f32) for s in DC.SHAPES.values() if s.form == "conv"}
    assert {(False, False, False, False), (True, False, False, False), (False, True, False, False), (False, False, True, False),
            (False, False, False, True), (True, True, True, False), (True, True, True, True)} <= epi


def test_padding_channels_and_neighbouring_records_are_poisoned():
    o = DC.operands("p11-cin10-all", "random")
    hi, lo = DC.plane_halves(o.xp)
    assert bool((hi[:, 10:] == DC.BIG).all()) and bool((lo[:, 10:] == DC.BIG).all()) and bool((hi[:, :10].abs() < DC.BIG).all())
    whi, wlo = DC.weight_halves(o.wp[0][0])
    assert torch.count_nonzero(whi[:, 10:]) == 0 and torch.count_nonzero(wlo[:, 10:]) == 0       # (through the packer: zero)
    for name in ("p11-wider", "p61-wider"):
        o = DC.operands(name, "random")
        (r0, n), total = o.slices[0], o.xp.shape[1]
        other = [r for r in range(total) if not r0 <= r < r0 + n]
        assert other and bool((o.xp[:, other].float() == DC.BIG).all())
        assert bool((o.xp[:, r0:r0 + n].float().abs() < DC.BIG).all())
