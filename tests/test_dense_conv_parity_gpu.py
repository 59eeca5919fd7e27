"""The dense 3x3 convolution on two fp16 planes per operand (csrc/dense_conv_wres.hip: hip.dense_conv3x3, and through it
hip.dense_conv3x3_wide and the SEW decoders' transposed convolution) on every route, per element, against the float64 references of
tests/dense_conv_cases.py.  Every case (shape x {exact, random} operands)

  * asserts through hip.launch_log() the list of launches - one per link: workgroups, threads, dynamic LDS (none), kernel with its
    template arguments - as the line dense_conv_cases.dispatch derives AND as the literal pinned in PINS below: a case meant for
    dense_conv_wres_kernel<6, 2> on the 256-workgroup grid that ran anything else fails here;
  * runs into an `out` that is a slice of a larger buffer, one guard image on each side, everything NaN beforehand: the guards hold
    the same bits afterwards and no NaN remains inside (the kernel stores through 2^31 - 1 byte buffer descriptors, nothing clamps a
    store one tile past the end; it writes every channel of every pixel, N being whole records - the format leaves nothing untouched);
    the planes, weights and residual it read are unchanged;
  * exact operands: the fp32 output, or the planes after hip.unpack_planes, are BIT-EQUAL to the fp64 result;
    random operands: |out - ref64| <= 2e-6 mag + floor + fmt for every element (dense_conv_cases' docstring; settled without a kernel by
    test_dense_conv_bound_cpu.py, where one missing cross product stands at 29 to 159 times the allowance);
  * runs twice: bit-equal;
  * the all-zero image is exactly act(beta + resid) - exact zeros without them - and the column with alpha = beta = 0 exactly
    act(resid) or 0.
The formats are not charged to the kernel and not taken on trust either: the planes the device's packers make (hip.pack_planes,
hip.pack_dense_conv_weight with its scale, hip.pack_planes_zero_up2) are asserted bit-equal to the CPU restatement the references read.

What the shapes are for: dense_conv_cases.SHAPES.

Measured on an MI355X, worst err / allowance over the single-launch random cases per kernel and grid (the CPU emulation's own
worst: 0.50 with plane output, where the store's 2^-22 meets fmt = 2^-21; 0.17 with fp32 output):
  <1,1>  partial 0.50   full 0.41        <6,1>  partial 0.49   full 0.42        <6,2>  partial 0.49   full 0.20
  fp32 outputs alone: p11-cin10-all 0.13, p61-f32 0.10, p61-all-f32 0.09, p62-f32 0.13, f62-n192 0.20, f11-walk 0.21;
  chains 0.37 (7 records), 0.41 (13), the transposed convolution 0.50; all 36 exact cases bit-equal.
Without the allowance's floor for fp16-subnormal halves (dense_conv_cases' docstring, "floor") two of these stood outside: f11-walk at
4.12 (9888 of 4.3 million elements, all in windows whose every activation is below 2^-14) and p61-f32 at 1.06 (4 elements); every
other case was where it is now.
Run time there: the 74 tests in 4.0 s; the first (it loads the library) 0.6 s, the four 256-workgroup shapes 0.06 to 0.21 s per
case with their fp64 reference, every other case 0.01 s.
"""
import functools

import pytest
import torch

import dense_conv_cases as DC
import routes_common
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = "dense_conv_wres_kernel"
P11, P61, P62 = f"768 0 {K}<1, 1>", f"768 0 {K}<6, 1>", f"512 0 {K}<6, 2>"
PINS = {
    "tiny-1x1x1-c16": [f"1 {P11}"], "tiny-1x2x3-c16": [f"1 {P11}"], "tiny-3x5x9-c16": [f"1 {P11}"], "tiny-2x4x8-c16": [f"1 {P11}"],
    "tiny-1x7x17-c16": [f"1 {P11}"], "tiny-5x3x31-c16": [f"2 {P11}"],
    "tiny-1x1x1-c96": [f"2 {P61}"], "tiny-1x2x3-c96": [f"2 {P61}"], "tiny-3x5x9-c96": [f"2 {P62}"], "tiny-2x4x8-c96": [f"2 {P61}"],
    "tiny-1x7x17-c96": [f"2 {P62}"], "tiny-5x3x31-c96": [f"4 {P61}"],
    "p11-none": [f"2 {P11}"], "p11-cin10-all": [f"6 {P11}"], "p11-wider": [f"1 {P11}"],
    "p61-none": [f"4 {P61}"], "p61-ab": [f"4 {P61}"], "p61-res": [f"4 {P61}"], "p61-relu": [f"4 {P61}"], "p61-f32": [f"4 {P61}"],
    "p61-all": [f"4 {P61}"], "p61-all-f32": [f"4 {P61}"], "p61-narrow": [f"2 {P61}"], "p61-wider": [f"3 {P61}"],
    "p62-all": [f"2 {P62}"], "p62-f32": [f"6 {P62}"], "p62-edges": [f"4 {P62}"],
    "p62-forced61": [f"2 {P61}"], "p61-forced62": [f"4 {P62}"],
    "f61-n96": [f"256 {P61}"], "f62-n192": [f"256 {P62}"], "f11-n64": [f"256 {P11}"], "f11-walk": [f"256 {P11}"],
    "chain-7": [f"4 {P61}", f"4 {P11}"], "chain-13": [f"3 {P62}", f"3 {P62}", f"3 {P11}"],
    "deconv-96-18": [f"1 {P61}", f"1 {P61}"],
}
WORST = {}                                       # single-launch random case -> ((kernel, grid), its worst err / allowance)


def _dev(t):
    return None if t is None else t.contiguous().to(DEV)


@functools.lru_cache(maxsize=4)
def _device(name, kind):
    """The case's device operands, made as the callers make them - and asserted to be, bit for bit, the planes the reference read."""
    o = DC.operands(name, kind)
    s = o.shape
    wsl = []
    for (r0, n), w, (planes, asc) in zip(o.slices, o.w, o.wp):
        wp = hip.pack_dense_conv_weight(_dev(w))
        assert torch.equal(wp.cpu(), planes) and wp.sdf_acc_scale == asc, "the device's weight planes are not the restated format"
        wsl.append(((r0, n), wp))
    if s.form == "deconv":                                                       # engine_sew._deconv_dense_fwd
        h, w_ = s.H // 2, s.W // 2
        xp = torch.full(o.xp.shape, DC.BIG, dtype=torch.float16, device=DEV)
        r0 = 0
        for p in o.parts:
            hip.pack_planes_zero_up2(_dev(p).reshape(s.imgs, h, w_, p.shape[-1]).permute(0, 3, 1, 2), xp, r0)
            r0 += DC.cdiv(p.shape[-1], 16)
        xp[:, r0:].zero_()
        assert torch.equal(xp.cpu(), o.xp), "pack_planes_zero_up2 is not the packed zero-upsampled image"
    else:
        assert torch.equal(hip.pack_planes(_dev(o.x)).cpu(), DC.pack_planes(o.x)), "the device's planes are not the restated format"
        xp = _dev(o.xp)                                                          # (with BIG in every record and channel that is not the operand's)
    resp = None
    if o.resid is not None:
        resp = hip.pack_planes(_dev(o.resid))
        assert torch.equal(resp.cpu(), o.resp)
    return xp, wsl, _dev(o.alpha), _dev(o.beta), resp


def _guarded(s):
    shape, dtype = ((s.imgs + 2, s.H, s.W, s.N), torch.float32) if s.f32 else ((s.imgs + 2, s.N // 16, s.H, s.W, 32), torch.float16)
    buf = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    bits = buf.view(torch.int32 if s.f32 else torch.int16)
    return buf, bits, int(bits.reshape(-1)[0])


def _run(name, kind):
    """One call into a guarded, NaN-filled `out` -> the result (imgs, N, H, W) fp32 on the CPU; the launch list, the guards, the
    inputs and where the result landed are asserted on the way."""
    o = DC.operands(name, kind)
    s = o.shape
    xp, wsl, alpha, beta, resp = _device(name, kind)
    buf, bits, nan_bits = _guarded(s)
    out = buf[1:-1]
    if s.form == "conv":
        (r0, n), wp = wsl[0]
        call = lambda: hip.dense_conv3x3(xp[:, r0:r0 + n], wp, alpha, beta, resp, s.relu, s.f32, out=out)
    else:
        call = lambda: hip.dense_conv3x3_wide(xp, wsl, beta, s.relu, s.f32, out=out)
    with hip.scoped_switches(SDF_DENSE_TPW=str(s.tpw_env) if s.tpw_env else None):
        launches, res = routes_common.logged(call)
    assert launches == DC.lines(name) == PINS[name], (launches, DC.lines(name), PINS[name])
    assert res.data_ptr() == out.data_ptr()
    assert bool((bits[0] == nan_bits).all()) and bool((bits[-1] == nan_bits).all()), "a store outside `out`"
    assert not bool(torch.isnan(out).any()), "an output element was never written"
    assert torch.equal(xp.cpu(), o.xp) and all(torch.equal(wp.cpu(), p) for (_, wp), (p, _) in zip(wsl, o.wp)), "an input was written"
    assert resp is None or torch.equal(resp.cpu(), o.resp), "the residual was written"
    return (out.permute(0, 3, 1, 2) if s.f32 else hip.unpack_planes(out, s.N)).cpu()


@pytest.mark.parametrize("name,kind", DC.CASES)
def test_dense_conv_per_element(name, kind):
    o, ref = DC.operands(name, kind), DC.reference(name, kind)
    s = o.shape
    assert all(hip.dense_conv_applicable(s.imgs, s.H, s.W, 16 * n, s.N) for _, n in o.slices)
    got = _run(name, kind)
    routes = DC.routes(name)
    tag = " + ".join(f"{r.kernel.replace(' ', '')} {'full' if r.full else 'partial'}" for r in routes)
    if kind == "exact":
        wrong = int((got.double() != ref["ref"]).sum())
        print(f"\nDENSECONV {tag} {name} exact: {wrong} of {got.numel()} elements differ")
        assert torch.equal(got.double(), ref["ref"]), wrong
    else:
        ratio = DC.ratio(got, name, kind)
        worst = ratio.max().item()
        if len(routes) == 1:
            WORST[name] = ((routes[0].kernel.replace(" ", ""), "full" if routes[0].full else "partial"), worst)
        print(f"\nDENSECONV {tag} {name} {worst:.2f}")
        assert bool((ratio <= 1.0).all()), worst
        # what no rounding explains: the silent image and the dead column, through the epilogue alone
        alone = DC.epilogue(torch.zeros(s.imgs, s.N, s.H, s.W), 1.0, o.alpha, o.beta, o.resp, s.relu, s.f32)
        if o.zero_img is not None:
            assert torch.equal(got[o.zero_img], alone[o.zero_img]), "the all-zero image is not act(beta + resid)"
            if o.beta is None and o.resid is None:
                assert torch.count_nonzero(got[o.zero_img]) == 0
        if o.zero_col is not None:
            assert torch.equal(got[:, o.zero_col], alone[:, o.zero_col]), "the alpha = beta = 0 column is not act(resid)"
    assert torch.equal(_run(name, kind), got), "two calls differ"


def test_worst_ratio_per_kernel_and_grid():
    """Prints the worst err / allowance of the single-launch random cases per kernel and grid (the file's docstring records it): what
    the cases above measured, or, run on its own, what it measures here.  Every instantiation is held on both grids."""
    for name in DC.SHAPES:
        if name not in WORST and len(DC.routes(name)) == 1:
            r = DC.routes(name)[0]
            WORST[name] = ((r.kernel.replace(" ", ""), "full" if r.full else "partial"), DC.ratio(_run(name, "random"), name, "random").max().item())
    table = {}
    for key, v in WORST.values():
        table[key] = max(table.get(key, 0.0), v)
    for (kernel, grid), v in sorted(table.items()):
        print(f"\nDENSECONV {kernel} {grid} {v:.2f}")
    assert set(table) == {(k, g) for k in ("<1,1>", "<6,1>", "<6,2>") for g in ("partial", "full")}
    assert max(table.values()) <= 1.0


def test_out_argument():
    """`out`: the result lands in it and is the fresh tensor's, bit for bit; a wrong shape, dtype or a strided tensor is refused."""
    o = DC.operands("p61-all", "random")
    s = o.shape
    xp, wsl, alpha, beta, resp = _device("p61-all", "random")
    wp = wsl[0][1]
    fresh = hip.dense_conv3x3(xp, wp, alpha, beta, resp, True, False)
    out = torch.zeros_like(fresh)
    assert hip.dense_conv3x3(xp, wp, alpha, beta, resp, True, False, out=out) is out and torch.equal(out, fresh)
    fresh32 = hip.dense_conv3x3(xp, wp, alpha, beta, resp, True, True)
    assert fresh32.shape == (s.imgs, s.H, s.W, s.N) and fresh32.dtype == torch.float32
    bad = [torch.zeros_like(fresh32),                                                            # the other format's shape and dtype
           torch.zeros((s.imgs, s.N // 16, s.H, s.W, 32), dtype=torch.float32, device=DEV),      # dtype
           torch.zeros((s.imgs + 1, s.N // 16, s.H, s.W, 32), dtype=torch.float16, device=DEV),  # shape
           torch.zeros((s.imgs, s.N // 16, s.H, s.W, 64), dtype=torch.float16, device=DEV)[..., ::2],   # strided
           torch.zeros(fresh.shape, dtype=torch.float16)]                                        # not on the device
    for b in bad:
        with pytest.raises(hip.SdfError):
            hip.dense_conv3x3(xp, wp, alpha, beta, resp, True, False, out=b)
    with pytest.raises(hip.SdfError):
        hip.dense_conv3x3(xp, wp, alpha, beta, resp, True, True, out=torch.zeros_like(fresh))
