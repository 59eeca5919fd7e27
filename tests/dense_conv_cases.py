"""Cases of the dense 3x3 convolution on two fp16 planes per operand (csrc/dense_conv_wres.hip, sdf_dense_conv3x3_fwd): shapes, operands,
float64 references, the per-element allowance, the launcher's dispatch restated, and a torch emulation of the kernel's arithmetic.
Plain CPU code, no GPU call in here; every builder is cached and nothing mutates what a builder returned.  Used by
test_dense_conv_bound_cpu.py (which fixes the tolerance and shows what it can see, without a kernel) and test_dense_conv_parity_gpu.py
(which holds the three instantiations to it).

  y[img, n, y, x] = act(alpha[n] * sum_{ky,kx,c} a[img, c, y+ky-1, x+kx-1] * w[n, c, ky, kx] + beta[n] (+ resid))

The formats, restated from the sources (the GPU file asserts that they are the device's planes bit for bit):
  activations  [img][record of 16 channels][H][W] x 4 pieces of {4 x hi, 4 x lo}: hi = fp16(x), lo = fp16(x - hi) (`pack_planes`);
  weights      (2, N, 144 records), K ordered (record, ky, kx, channel in record): hi / lo of s * w, s the power of two that puts
               max |w| into [2^14, 2^15); 1 / s multiplies the accumulator (`weight_planes` = hip._f16_planes).

Two kinds of operands per shape.

exact   The float64 result is the fp32 result in any summation order, so the kernel's output must be bit-equal to it: the geometry
        test - a wrong tap, border, image wrap, record or column block shows at any magnitude.  Two nonzero channels per pixel.  On
        EVEN channels the activation has two terms and the weight one: a = +-(h / 4 + l 2^-12), h in 4..7, l = +-1 (hi = h / 4,
        lo = +-2^-12), w = +-2^e {1, 1.5}, e in -3..0 (lo plane zero).  On ODD channels it is the other way round: a = +-h / 4,
        w = +-2^e ({1, 1.5} + l 2^-12), e in -2..0 (under the packer's scale 2^14: lo = +-2^(2+e)).  a_lo * w_lo, the product the
        kernel drops, is then exactly zero, and every product is a multiple of 2^-16.  alpha is +-1, 2 or 0.5; beta a multiple of 2^-4
        within +-2; resid = +-(h / 4 + l 2^-12).  `assert_exact` checks on the CPU that every element's magnitude sum over its unit
        |alpha| 2^-16 stays below 2^24 (fp32 output) or 2^22 (what hi + lo holds), and that every nonzero half of every operand is
        a normal fp16 number (the exact cases do not lean on subnormals).
random  randn activations times a scale 10^(2 - 9 u) that is constant over blocks of 3 x 5 pixels, u uniform: 1e-7 .. 1e2, so whole
        windows have fp16-subnormal hi halves; one image all zero; weights randn / (3 sqrt(Cin)); alpha in (0.5, 1.5), every fifth
        negative; one output column with alpha = beta = 0; beta, resid randn.  The reference is fp64 on the values the planes HOLD
        (hi + lo of the activations and the residual, (hi + lo) / s of the weights), so the formats' rounding is not charged to
        the kernel.  Per element

            |out - ref64| <= TOL * mag + floor + fmt,    mag = |alpha| conv(|a|, |w|) + |beta| + |resid|,

        fmt = 2^-21 |ref| + 2^-24 where the result is stored as planes (the hi + lo store; fp16 has the fixed spacing 2^-24 below
        2^-14) and 0 for fp32 output; a chain adds one such term per intermediate link (its result is stored as planes and read back
        as the next link's residual).
floor   The held-value reference removes what the formats round away - among it the 2^-24 spacing of a subnormal half's VALUE.  It
        does not remove this: an fp16 number below 2^-14 still CARRIES the exponent 2^-14 (a subnormal is 0.xxx * 2^-14, no hidden
        bit), and a multiply-accumulate unit aligns and rounds its sum by the exponents of the terms, not by their values.  TOL is a
        bound relative to every term's magnitude; for a term with a subnormal half that magnitude is, to the hardware, 2^-14 times
        the other factor.  So floor = TOL * (|alpha| conv(a', w') - |alpha| conv(|a|, |w|)), a' = sum over the two halves of
        max(|half|, 2^-14) where the half is not zero (likewise w', in the packer's scaled domain).  For |a| >= 2^-3 both halves are
        normal and the floor is nothing; a pixel at 1e-3 gains 6 %; a window of activations at 1e-7 is held to 2e-6 * 2^-14 * sum |w|
        instead of 2e-6 * 1e-7 * sum |w| - 1 / 500 of the 2^-25 sum |w| that test_dense_linear_gpu.py grants the same arithmetic.
        The form and the constant come from the format alone.  Why it is here at all: the first version of this module had no floor
        (the argument being that the reference already contains the subnormal spacing), and gfx950 missed it on fp32 outputs whose
        whole window is subnormal, at up to 4.1 x (f11-walk; 1.06 x on p61-f32), everything else inside.  Read off those outputs: the
        error there is one-sided (98 % of the elements BELOW the reference) and of one absolute size, about 2^-21 of the largest
        weight whatever the result's own magnitude - the signature of a sum aligned by exponent fields and truncated, which is what
        the paragraph above allows for; that the matrix cores do exactly this is a supposition.  With the floor the flushed-subnormal
        fault still stands at 2.3 to 1e5 times the allowance (test_dense_conv_bound_cpu.py).

TOL = 2e-6, the project's per-element bound for this three-product arithmetic (test_dense_linear_gpu.py, K up to 1536), kept as it
is.  The emulation below - fp16 halves, the kernel's three products in its order, fp32 sums per 16-channel step and tap, fp32
epilogue, the plane store - confirms it and shows NO tighter constant: its worst (|err| - fmt) / mag over the random cases is
E_EMU = 4.1e-7 (f11-walk: 4.3 million fp32 outputs of 27 accumulations each; recorded here, recomputed and held within a factor 3 by
test_dense_conv_bound_cpu.py), and 8 x that - the factor of ann_block_cases.R32 - is 3.3e-6, above 2e-6.  So the emulation uses at most
0.21 of TOL * mag where the result is fp32, and 0.50 of the allowance where the plane store's own 2^-22 meets fmt = 2^-21.  Nothing is fitted
to a kernel.
"""
import functools
import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

TW, NB = 8, 32                                   # pixels of a tile row; output columns of a workgroup
BIG = 1.0e4                                      # what records and channels the kernel must not read are filled with
TOL = 2e-6                                       # test_dense_linear_gpu.py's per-element constant
E_EMU = 4.1e-07                                  # worst (|emulation - ref64| - fmt) / mag over the random cases (test_dense_conv_bound_cpu.py)
assert 8.0 * E_EMU > TOL                         # the emulation shows no tighter constant: TOL stays the project's


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the launcher's dispatch, restated
@dataclass(frozen=True)
class Route:
    cch: int
    tpw: int
    NW: int
    TH: int
    ncb: int
    wtiles: int
    want: int
    ranges: int
    G: int

    @property
    def full(self):
        return self.G == 256

    @property
    def kernel(self):
        return f"<{self.cch}, {self.tpw}>"

    @property
    def line(self):
        """The launch in routes_common.logged notation; the kernel's LDS is static."""
        return f"{self.G} {64 * self.NW} 0 dense_conv_wres_kernel<{self.cch}, {self.tpw}>"


def dispatch(imgs, H, W, cin_records, N, tpw_env=0):
    """sdf_dense_conv3x3_fwd's choice of instantiation and grid: two pixel blocks per wave where 8-row tiles waste no more rows than
    4-row tiles (or the map is at least 128 rows), SDF_DENSE_TPW = 1 | 2 overrides for six records; a workgroup wants a tile per wave;
    256 / ncb ranges at most, and then the grid is the whole 256."""
    assert cin_records in (1, 6) and N % NB == 0 and N // NB <= 32
    ncb = N // NB
    waste8, waste4 = cdiv(H, 8) * 8 - H, cdiv(H, 4) * 4 - H
    tpw = 2 if cin_records == 6 and (waste8 == waste4 or H >= 128) else 1
    if cin_records == 6 and tpw_env in (1, 2):
        tpw = tpw_env
    TH, NW = 4 * tpw, (12 if tpw == 1 else 8)
    wtiles = imgs * cdiv(H, TH) * cdiv(W, TW)
    want = cdiv(wtiles, NW)
    ranges = min(want, 256 // ncb)
    G = 256 if ranges == 256 // ncb else ranges * ncb
    return Route(cin_records, tpw, NW, TH, ncb, wtiles, want, ranges, G)


def workgroups(r: Route):
    """[(range, column block, branch)] per workgroup id - the kernel's remap: on the 256-workgroup grid workgroup p is the (p / 8)-th
    of XCD p % 8; each XCD serves m = 32 / ncb whole ranges ("whole") and the 32 - m ncb workgroups left over are pooled across the
    XCDs ("pooled"); a pooled workgroup beyond the last range returns ("surplus").  Any other grid: range = id / ncb ("linear")."""
    out = []
    for b in range(r.G):
        if r.G == 256 and r.ncb <= 32:
            x, k, m = b & 7, b >> 3, 32 // r.ncb
            if k < m * r.ncb:
                rng, cb, branch = x * m + k // r.ncb, k % r.ncb, "whole"
            else:
                e = x * (32 - m * r.ncb) + (k - m * r.ncb)
                rng, cb, branch = 8 * m + e // r.ncb, e % r.ncb, "pooled"
        else:
            rng, cb, branch = b // r.ncb, b % r.ncb, "linear"
        out.append((rng, cb, branch if rng < r.ranges else "surplus"))
    return out


def walk(r: Route, H, W):
    """{"items": tiles per wave, over all (range, wave); "tiles": every (img, ty, tx) a wave multiplies, through the kernel's
    pos_of / advance}: a wave starts at tile t_begin + wave and advances by NW tile columns, wrapping over rows and images."""
    tiles_x, tiles_y = cdiv(W, TW), cdiv(H, r.TH)
    base, rem = divmod(r.wtiles, r.ranges)
    items, tiles = [], []
    for rng in range(r.ranges):
        t_begin, n_my = rng * base + min(rng, rem), base + (1 if rng < rem else 0)
        for wave in range(r.NW):
            n = cdiv(n_my - wave, r.NW) if n_my > wave else 0
            items.append(n)
            t = t_begin + wave
            img, tl = divmod(t, tiles_x * tiles_y)
            ty, tx = divmod(tl, tiles_x)
            for _ in range(n):
                tiles.append((img, ty, tx))
                tx += r.NW
                while tx >= tiles_x:
                    tx -= tiles_x
                    ty += 1
                while ty >= tiles_y:
                    ty -= tiles_y
                    img += 1
    return {"items": items, "tiles": tiles}


def interior(r: Route, H, W, ty, tx):
    """The halo loader's fast path: every pixel of the tile's halo exists."""
    y0, x0 = ty * r.TH, tx * TW
    return y0 >= 1 and x0 >= 1 and y0 + r.TH + 1 <= H and x0 + TW + 1 <= W


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Shape:
    imgs: int
    Cin: int                                     # conv / chain: input channels; deconv: unused (see parts)
    N: int
    H: int
    W: int
    affine: bool = False                         # alpha and beta (chain / deconv: beta only, the last link's bias)
    resid: bool = False
    relu: bool = False
    f32: bool = False
    tpw_env: int = 0                             # SDF_DENSE_TPW
    wider: tuple = None                          # (records of the wider planes tensor, first record of the operand)
    form: str = "conv"                           # "conv": one call; "chain": dense_conv3x3_wide; "deconv": the SEW decoders' form
    parts: tuple = None                          # deconv: channels of the channels-last parts; H, W are the OUTPUT size (even)


S = Shape
SHAPES = {
    # --- the maps of tools/probes/dense_tiny_shapes.py, for one record and for six (all partial grids, all edge tiles, most waves idle)
    "tiny-1x1x1-c16": S(1, 16, 32, 1, 1),                              # one pixel: every tap but the centre is padding
    "tiny-1x2x3-c16": S(1, 16, 32, 2, 3),
    "tiny-3x5x9-c16": S(3, 16, 32, 5, 9),                              # 12 tiles, one range: S = 1 (odd) on every wave
    "tiny-2x4x8-c16": S(2, 16, 32, 4, 8),                              # exactly one whole tile per image
    "tiny-1x7x17-c16": S(1, 16, 32, 7, 17),
    "tiny-5x3x31-c16": S(5, 16, 32, 3, 31),                            # 20 tiles: two ranges of 10, waves 10 and 11 idle
    "tiny-1x1x1-c96": S(1, 96, 64, 1, 1),
    "tiny-1x2x3-c96": S(1, 96, 64, 2, 3),
    "tiny-3x5x9-c96": S(3, 96, 64, 5, 9),                              # H 5: 8-row tiles waste as much as 4-row ones -> <6,2>
    "tiny-2x4x8-c96": S(2, 96, 64, 4, 8),
    "tiny-1x7x17-c96": S(1, 96, 64, 7, 17),                            # <6,2>, three tiles of which rows 7 are padding
    "tiny-5x3x31-c96": S(5, 96, 64, 3, 31),
    # --- every instantiation on the partial grid, by the rule and forced; epilogues
    "p11-none": S(2, 16, 64, 9, 16),                                   # <1,1>; 12 tiles in one range; no epilogue
    "p11-cin10-all": S(2, 10, 96, 13, 21, True, True, True, True),     # 6 padding channels (filled with BIG); H, W ragged; 3 column blocks
    "p11-wider": S(3, 16, 32, 6, 11, True, False, False, False, 0, (5, 3)),      # record 3 of 5, the others BIG
    "p61-none": S(2, 96, 64, 12, 20),                                  # <6,1> by the rule (H 12: 8-row tiles would waste 4); interior tile (1, 1)
    "p61-ab": S(2, 96, 64, 12, 20, True),
    "p61-res": S(2, 96, 64, 12, 20, False, True),                      # the residual of the second column block must not be the first's
    "p61-relu": S(2, 96, 64, 12, 20, False, False, True),
    "p61-f32": S(2, 96, 64, 12, 20, False, False, False, True),        # fp32 channels-last against planes (p61-none)
    "p61-all": S(2, 96, 64, 12, 20, True, True, True),
    "p61-all-f32": S(2, 96, 64, 12, 20, True, True, True, True),
    "p61-narrow": S(5, 96, 32, 12, 7, True, True),                     # tiles_x = 1 < NW: a range's waves span tile rows and images
    "p61-wider": S(2, 96, 96, 4, 19, False, False, True, False, 0, (8, 1)),      # records 1..6 of 8, the others BIG; two images
    "p62-all": S(1, 96, 32, 24, 24, True, True, True),                 # <6,2> by the rule; 9 tiles in ranges of 5 and 4: idle waves; interior (1, 1)
    "p62-f32": S(2, 96, 96, 13, 21, False, False, False, True),        # H 13: rows 13..15 of the lower tiles are padding
    "p62-edges": S(3, 96, 64, 16, 16, True),                           # two tile rows, two columns: edge tiles only
    "p62-forced61": S(1, 96, 32, 24, 24, True, True, True, False, 1),  # SDF_DENSE_TPW=1 where the rule picks <6,2>
    "p61-forced62": S(2, 96, 64, 12, 20, True, True, True, False, 2),  # SDF_DENSE_TPW=2 where the rule picks <6,1>: rows 12..15 padding
    # --- every instantiation on the 256-workgroup grid, wtiles % ranges != 0
    "f61-n96": S(38, 96, 96, 36, 24, True, True, True),                # 1026 tiles, 85 ranges (ncb 3: pooled branch, one surplus workgroup); ranges 0..5
                                                                       # hold 13 tiles: wave 0 advances over 4 tile rows; interior tiles
    "f62-n192": S(57, 96, 192, 16, 24, True, False, True, True),       # 342 tiles, 42 ranges (ncb 6: pooled, four surplus); ranges 0..5 hold 9
    "f11-n64": S(129, 16, 64, 11, 30, True, True),                     # 1548 tiles, 128 ranges (ncb 2 divides 32: no pooled branch); S = 1 and 2
    "f11-walk": S(401, 16, 256, 6, 7, False, False, True, True),       # tiles_x = 1: 802 tiles, 32 ranges of 25 / 26: S = 3 (odd) and 2, advance crosses
                                                                       # 12 tile rows = 6 images a step; ranges begin in the middle of an image
    # --- chains (hip.dense_conv3x3_wide): bias, ReLU, fp32 output
    "chain-7": S(2, 100, 64, 12, 20, True, False, True, True, 0, None, "chain"),       # 6 + 1 records, 12 padding channels
    "chain-13": S(2, 194, 96, 8, 12, True, False, True, True, 0, None, "chain"),       # 6 + 6 + 1 (the decoders' 194 channels)
    # --- the SEW decoders' transposed convolution: parts 96 + 18 channels -> 6 + 2 records, rounded up to 12 by four zero records
    "deconv-96-18": S(2, 0, 32, 10, 14, False, False, False, True, 0, None, "deconv", (96, 18)),
}
KINDS = ("exact", "random")
CASES = [(n, k) for n in SHAPES for k in KINDS]


def records_of(s: Shape):
    """(records of the planes tensor, [(first record, count)] of the links)."""
    if s.form == "conv":
        n = cdiv(s.Cin, 16)
        return (s.wider[0], [(s.wider[1], n)]) if s.wider else (n, [(0, n)])
    total = cdiv(s.Cin, 16) if s.form == "chain" else sum(cdiv(c, 16) for c in s.parts)
    while total % 6 > 1:
        total += 1
    six, one = divmod(total, 6)                                                  # hip.dense_conv_slices
    return total, [(6 * i, 6) for i in range(six)] + ([(6 * six, 1)] if one else [])


def routes(name):
    """One Route per link of the case's call."""
    s = SHAPES[name]
    return [dispatch(s.imgs, s.H, s.W, n, s.N, s.tpw_env) for _, n in records_of(s)[1]]


def lines(name):
    return [r.line for r in routes(name)]


# ------------------------------------------------------------------------------------------------ the formats
def pack_planes(x):
    """(imgs, C, H, W) fp32 -> (imgs, ceil(C / 16), H, W, 32) fp16 (sdf_pack_planes restated); channels beyond C are zero."""
    imgs, C, H, W = x.shape
    rec = cdiv(C, 16)
    xp = F.pad(x, (0, 0, 0, 0, 0, rec * 16 - C))
    hi = xp.half()
    lo = (xp - hi.float()).half()
    t = torch.stack([hi, lo]).view(2, imgs, rec, 4, 4, H, W)                      # [half, img, record, piece, element, y, x]
    return t.permute(1, 2, 5, 6, 3, 0, 4).reshape(imgs, rec, H, W, 32).contiguous()


def plane_halves(p):
    """planes -> (hi, lo), each (imgs, 16 records, H, W) fp32."""
    imgs, rec, H, W, _ = p.shape
    t = p.float().view(imgs, rec, H, W, 4, 2, 4).permute(5, 0, 1, 4, 6, 2, 3).reshape(2, imgs, rec * 16, H, W)
    return t[0], t[1]


def weight_planes(w):
    """(N, Cin, 3, 3) fp32 -> ((2, N, 144 records) fp16, 1 / scale): hip.pack_dense_conv_weight and hip._f16_planes restated."""
    N, Cin = w.shape[:2]
    rec = cdiv(Cin, 16)
    wk = F.pad(w.float(), (0, 0, 0, 0, 0, rec * 16 - Cin)).view(N, rec, 16, 3, 3).permute(0, 1, 3, 4, 2).reshape(N, rec * 144)
    mx = float(wk.abs().max())
    scale = 2.0 ** (14 - math.floor(math.log2(mx))) if mx > 0 else 1.0
    ws = wk * scale
    hi = ws.half()
    return torch.stack([hi, (ws - hi.float()).half()]).contiguous(), 1.0 / scale


def weight_halves(wp):
    """weight planes -> (hi, lo), each (N, 16 records, 3, 3) fp32, in the scaled domain."""
    N, rec = wp.shape[1], wp.shape[2] // 144
    t = wp.float().view(2, N, rec, 3, 3, 16).permute(0, 1, 2, 5, 3, 4).reshape(2, N, rec * 16, 3, 3)
    return t[0], t[1]


def store_planes(o):
    """What the plane store keeps of an fp32 result: hi + lo (piece_from / piece_to of the kernel file)."""
    hi = o.half().float()
    return hi + (o - hi).half().float()


# ------------------------------------------------------------------------------------------------ operands
@dataclass
class Ops:
    name: str
    kind: str
    shape: Shape
    x: torch.Tensor                              # (imgs, C, H, W) fp32 in PHYSICAL channel order, before packing (deconv: the zero-upsampled image)
    creal: list                                  # physical channels that carry data (the others are padding)
    xp: torch.Tensor                             # the planes tensor the call reads, BIG in every record and channel it must not use
    slices: list                                 # [(first record, count)]
    w: list                                      # per link (N, 16 count, 3, 3) fp32
    wp: list                                     # per link (planes, 1 / scale)
    alpha: torch.Tensor
    beta: torch.Tensor
    resid: torch.Tensor                          # (imgs, N, H, W) fp32 before packing, or None
    resp: torch.Tensor                           # its planes
    zero_img: int                                # the all-zero image, or None
    zero_col: int                                # the output column with alpha = beta = 0, or None
    parts: list = None                           # deconv: the channels-last (imgs, h, w, c) parts
    wdec: torch.Tensor = None                    # deconv: the ConvTranspose2d weight (sum of parts, N, 3, 3)
    ref: dict = field(default_factory=dict)


def _two_term(shape, g):
    """+-(h / 4 + l 2^-12), h in 4..7, l = +-1: hi = h / 4, lo = +-2^-12."""
    h = torch.randint(4, 8, shape, generator=g).float() / 4.0
    l = (torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0) * 2.0 ** -12
    sg = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    return sg * (h + l), sg * h


def _exact_x(imgs, C, H, W, g):
    even = 2 * torch.randint(0, cdiv(C, 2), (imgs, 1, H, W), generator=g)         # one channel of each set per pixel
    picks = torch.cat([even, 2 * torch.randint(0, C // 2, (imgs, 1, H, W), generator=g) + 1], 1)
    two, one = _two_term((imgs, 2, H, W), g)
    val = torch.where(picks % 2 == 0, two, one)
    return torch.zeros(imgs, C, H, W).scatter_(1, picks, val)


def _exact_w(N, C, g):
    shape = (N, C, 3, 3)
    sig = 1.0 + 0.5 * torch.randint(0, 2, shape, generator=g).float()
    l = (torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0) * 2.0 ** -12
    sg = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    odd = (torch.arange(C) % 2 == 1).view(1, C, 1, 1)
    e = torch.where(odd, torch.randint(-2, 1, shape, generator=g), torch.randint(-3, 1, shape, generator=g)).float()
    return sg * torch.exp2(e) * torch.where(odd, sig + l, sig)


def _random_x(imgs, C, H, W, g):
    u = torch.rand(imgs, 1, cdiv(H, 3), cdiv(W, 5), generator=g)
    u = u.repeat_interleave(3, 2).repeat_interleave(5, 3)[:, :, :H, :W]
    return torch.randn(imgs, C, H, W, generator=g) * 10.0 ** (2.0 - 9.0 * u)


@functools.lru_cache(maxsize=None)
def operands(name, kind):
    s = SHAPES[name]
    g = torch.Generator().manual_seed(7000 + 10 * list(SHAPES).index(name) + KINDS.index(kind))
    total, slices = records_of(s)
    exact = kind == "exact"
    zero_img = s.imgs // 2 if (not exact and s.imgs >= 2) else None
    parts = wdec = None
    if s.form == "deconv":
        h, w_ = s.H // 2, s.W // 2
        cs = list(s.parts)
        ctot = sum(cs)
        xr = _exact_x(s.imgs, ctot, h, w_, g) if exact else _random_x(s.imgs, ctot, h, w_, g)
        wdec = (_exact_w(s.N, ctot, g) if exact else torch.randn(s.N, ctot, 3, 3, generator=g) / (3.0 * ctot ** 0.5)).permute(1, 0, 2, 3).contiguous()
        if zero_img is not None:
            xr[zero_img] = 0.0
        x = torch.zeros(s.imgs, total * 16, s.H, s.W)
        wphys = torch.zeros(total * 16, s.N, 3, 3)
        parts, creal, c0, r0 = [], [], 0, 0
        for c in cs:                                                             # every part starts on a record (engine_sew._deconv_dense_fwd)
            parts.append(xr[:, c0:c0 + c].permute(0, 2, 3, 1).contiguous())
            x[:, 16 * r0:16 * r0 + c, ::2, ::2] = xr[:, c0:c0 + c]
            wphys[16 * r0:16 * r0 + c] = wdec[c0:c0 + c]
            creal += list(range(16 * r0, 16 * r0 + c))
            c0, r0 = c0 + c, r0 + cdiv(c, 16)
        wconv = wphys.flip(2, 3).permute(1, 0, 2, 3).contiguous()                # the equivalent correlation
        xp = pack_planes(x)                                                      # (zero records and padding channels are ZERO here, as the engine leaves them)
    else:
        x = _exact_x(s.imgs, s.Cin, s.H, s.W, g) if exact else _random_x(s.imgs, s.Cin, s.H, s.W, g)
        if zero_img is not None:
            x[zero_img] = 0.0
        wconv = _exact_w(s.N, s.Cin, g) if exact else torch.randn(s.N, s.Cin, 3, 3, generator=g) / (3.0 * s.Cin ** 0.5)
        creal = list(range(s.Cin))
        own = pack_planes(x)
        n = own.shape[1]
        pad = own.view(s.imgs, n, s.H, s.W, 4, 2, 4)                             # padding channels of the last record: BIG, not zero
        for c in range(s.Cin, n * 16):
            pad[:, -1, :, :, (c % 16) // 4, :, c % 4] = BIG
        xp = torch.full((s.imgs, total, s.H, s.W, 32), BIG, dtype=torch.float16)
        first = slices[0][0]
        xp[:, first:first + n] = own
        x = F.pad(x, (0, 0, 0, 0, 0, n * 16 - s.Cin))
        wconv = F.pad(wconv, (0, 0, 0, 0, 0, n * 16 - s.Cin))
    first = slices[0][0]
    w = [wconv[:, 16 * (r0 - first):16 * (r0 - first + n)].contiguous() for r0, n in slices]
    alpha = beta = resid = None
    zero_col = None
    if s.affine:
        if exact:
            alpha = torch.tensor([1.0, 2.0, -1.0, 0.5])[torch.randint(0, 4, (s.N,), generator=g)]
            beta = torch.randint(-32, 33, (s.N,), generator=g).float() / 16.0
        else:
            alpha = 0.5 + torch.rand(s.N, generator=g)
            alpha[::5] *= -1.0
            beta = torch.randn(s.N, generator=g)
            zero_col = s.N // 2 + 1
            alpha[zero_col] = beta[zero_col] = 0.0
        if s.form != "conv":
            alpha, zero_col = None, None                                         # a chain has no alpha; beta is the last link's bias
    if s.resid:
        resid = _two_term((s.imgs, s.N, s.H, s.W), g)[0] if exact else torch.randn(s.imgs, s.N, s.H, s.W, generator=g)
    return Ops(name, kind, s, x, creal, xp, slices, w, [weight_planes(wk) for wk in w], alpha, beta, resid,
               None if resid is None else pack_planes(resid), zero_img, zero_col, parts, wdec)


# ------------------------------------------------------------------------------------------------ references
def _held(o: Ops):
    """The values the planes hold, fp64: activations (imgs, C, H, W) over the links' records with ONLY the real channels kept, weights
    per link, residual."""
    first, last = o.slices[0][0], o.slices[-1][0] + o.slices[-1][1]
    hi, lo = plane_halves(o.xp[:, first:last])
    xh = hi.double() + lo.double()
    keep = torch.zeros(xh.shape[1], dtype=torch.bool)
    keep[o.creal] = True
    xh = xh * keep.view(1, -1, 1, 1)
    wh = []
    for wp, asc in o.wp:
        hi, lo = weight_halves(wp)
        wh.append((hi.double() + lo.double()) * asc)
    rh = None
    if o.resp is not None:
        hi, lo = plane_halves(o.resp)
        rh = hi.double() + lo.double()
    return xh, wh, rh


def reference(name, kind):
    """{"ref", "mag", "floor", "fmt", "partial"} of one case, fp64, (imgs, N, H, W): computed once, shared, never modified."""
    o = operands(name, kind)
    if o.ref:
        return o.ref
    s = o.shape
    xh, wh, rh = _held(o)
    first = o.slices[0][0]
    cut = [(16 * (r0 - first), 16 * (r0 - first + n)) for r0, n in o.slices]
    partial, acc = [], None
    for (a, b), wk in zip(cut[:-1], wh[:-1]):                                    # what every intermediate link leaves as planes
        y = F.conv2d(xh[:, a:b], wk, None, 1, 1)
        acc = y if acc is None else acc + y
        partial.append(acc)
    wcat = torch.cat(wh, 1)
    if s.form == "deconv":                                                       # the whole against the transposed convolution itself
        small = xh[:, :, ::2, ::2]
        assert torch.count_nonzero(xh) == torch.count_nonzero(small)
        y = F.conv_transpose2d(small, wcat.permute(1, 0, 2, 3).flip(2, 3), None, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(xh, wcat, None, 1, 1)
    mag = F.conv2d(xh.abs().float(), wcat.abs().float(), None, 1, 1).double()    # (a scale: fp32 is plenty)
    # the same sum with every nonzero half at no less than 2^-14, the exponent an fp16 subnormal carries (the module docstring: floor)
    nominal = lambda hi, lo: sum(torch.where(h != 0, h.abs().clamp_min(2.0 ** -14), h.abs()) for h in (hi, lo))
    first, end = o.slices[0][0], o.slices[-1][0] + o.slices[-1][1]
    xn = nominal(*plane_halves(o.xp[:, first:end])) * (xh != 0)                  # (real channels only)
    wn = torch.cat([nominal(*weight_halves(wp)) * asc for wp, asc in o.wp], 1)
    floor = TOL * (F.conv2d(xn.float(), wn.float(), None, 1, 1).double() - mag).clamp_min(0.0)
    col = lambda v: v.double().view(1, -1, 1, 1)
    if o.alpha is not None:
        y, mag, floor = y * col(o.alpha), mag * col(o.alpha).abs(), floor * col(o.alpha).abs()
    if o.beta is not None:
        y, mag = y + col(o.beta), mag + col(o.beta).abs()
    if rh is not None:
        y, mag = y + rh, mag + rh.abs()
    if s.relu:
        y = torch.relu(y)
    plane = lambda v: 2.0 ** -21 * v.abs() + 2.0 ** -24
    fmt = torch.zeros_like(y) if s.f32 else plane(y)
    for p in partial:
        fmt = fmt + plane(p)
    o.ref.update(ref=y, mag=mag, floor=floor, fmt=fmt, partial=partial)
    return o.ref


def assert_exact(name):
    """The promises of an `exact` case, on the CPU: the fp64 result is an fp32 number, every element's magnitude sum over its unit fits
    the output format (24 bits fp32, 22 bits hi + lo; intermediate links of a chain: 22), every nonzero half is a normal fp16 number,
    and the product the kernel drops is zero."""
    o, r = operands(name, "exact"), reference(name, "exact")
    s = o.shape
    assert torch.equal(r["ref"].float().double(), r["ref"])
    unit = 2.0 ** -16 * (torch.ones(s.N, dtype=torch.float64) if o.alpha is None else o.alpha.double().abs()).view(1, -1, 1, 1)
    assert torch.equal(torch.round(r["ref"] / unit) * unit, r["ref"]), "the result is not on its grid"
    bits = torch.log2((r["mag"] / unit).max()).item()
    assert bits < (24 if s.f32 else 22), bits
    if r["partial"]:
        assert torch.log2(r["mag"].max() / 2.0 ** -16).item() < 22                # (a chain has no alpha: mag bounds every partial sum)
    halves = [*plane_halves(o.xp[:, o.slices[0][0]:o.slices[-1][0] + o.slices[-1][1]])]
    halves += [h for wp, _ in o.wp for h in weight_halves(wp)]
    if o.resp is not None:
        halves += [*plane_halves(o.resp)]
    for h in halves:
        nz = h[h != 0].abs()
        assert nz.numel() == 0 or (nz.min().item() >= 2.0 ** -14 and nz.max().item() <= 65504.0)
    xh, xl = plane_halves(o.xp[:, o.slices[0][0]:o.slices[-1][0] + o.slices[-1][1]])
    wl = torch.cat([weight_halves(wp)[1] for wp, _ in o.wp], 1)
    lolo = (xl[:, o.creal] != 0).any(0).any(-1).any(-1) & (wl[:, o.creal] != 0).any(0).any(-1).any(-1)     # per channel: both lo halves in use
    assert not bool(lolo.any())
    assert bool((xl[:, o.creal] != 0).any()) and bool((wl != 0).any())            # and both lo planes are in use somewhere
    return bits


def ratio(out, name, kind):
    """err / allowance per element for a result `out` (imgs, N, H, W); an element with no allowance must be exact."""
    r = reference(name, kind)
    err = (out.double() - r["ref"]).abs()
    allow = TOL * r["mag"] + r["floor"] + r["fmt"]
    return torch.where(err == 0, torch.zeros_like(err), err / allow)


def err_over_mag(out, name, kind):
    """max (|out - ref| - fmt)+ / mag: the part of the error the format's store does not explain, per unit of magnitude."""
    r = reference(name, kind)
    err = ((out.double() - r["ref"]).abs() - r["fmt"]).clamp_min(0.0)
    return torch.where(err == 0, torch.zeros_like(err), err / r["mag"]).max().item()


# ------------------------------------------------------------------------------------------------ emulation of the kernel's arithmetic
def epilogue(acc, asc, alpha, beta, resp, relu, f32):
    """The kernel's epilogue on the accumulator (imgs, N, H, W) fp32: fma(acc, alpha / s, beta), + hi + lo of the residual, ReLU, and
    the store (fp32, or hi + lo)."""
    N = acc.shape[1]
    al = (torch.full((N,), asc) if alpha is None else alpha * asc).view(1, -1, 1, 1)          # 1 / s is a power of two
    be = (torch.zeros(N) if beta is None else beta).view(1, -1, 1, 1)
    o = (acc.double() * al.double() + be.double()).float()                       # one rounding, as the fused multiply-add
    if resp is not None:
        hi, lo = plane_halves(resp)
        o = o + (hi + lo)
    if relu:
        o = torch.relu(o)
    return o if f32 else store_planes(o)


@functools.lru_cache(maxsize=None)
def tap_pixel(name, kind):
    """Flat index (img, y, x) of the border pixel whose own activations are the largest: where the "tap" fault drops the centre tap."""
    o = operands(name, kind)
    s = o.shape
    own = o.x.abs().sum(1)
    border = torch.zeros(s.H, s.W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    return int((own * border).reshape(-1).argmax())


def emulate(name, kind, fault=None):
    """The call's result (imgs, N, H, W) fp32 in the kernel's arithmetic: per link, per 16-channel record, per tap, three matrix
    products in the kernel's order - w_hi a_lo, w_lo a_hi, w_hi a_hi - each an fp32 sum over 16 channels added to the fp32 accumulator.
    fault: "no_alo_whi" / "no_wlo_ahi" (one cross product missing), "ftz" (fp16 subnormal halves read as zero), "tap" (the centre tap
    dropped at one border pixel, `tap_pixel`), "resid_cb" (the residual read from the next column block)."""
    o = operands(name, kind)
    s = o.shape
    ftz = lambda v: torch.where(v.abs() < 2.0 ** -14, torch.zeros_like(v), v) if fault == "ftz" else v
    res = None
    for k, ((r0, n), (wp, asc)) in enumerate(zip(o.slices, o.wp)):
        last = k == len(o.slices) - 1
        xh, xl = (F.pad(ftz(h), (1, 1, 1, 1)) for h in plane_halves(o.xp[:, r0:r0 + n]))
        wh, wl = (ftz(h) for h in weight_halves(wp))
        acc = torch.zeros(s.imgs * s.H * s.W, s.N)
        for rec in range(n):
            c = slice(16 * rec, 16 * rec + 16)
            for ky in range(3):
                for kx in range(3):
                    ah = xh[:, c, ky:ky + s.H, kx:kx + s.W].permute(0, 2, 3, 1).reshape(-1, 16)
                    al = xl[:, c, ky:ky + s.H, kx:kx + s.W].permute(0, 2, 3, 1).reshape(-1, 16)
                    if fault == "tap" and (ky, kx) == (1, 1):
                        ah, al = ah.clone(), al.clone()
                        ah[tap_pixel(name, kind)] = al[tap_pixel(name, kind)] = 0.0
                    bh, bl = wh[:, c, ky, kx].T.contiguous(), wl[:, c, ky, kx].T.contiguous()
                    if fault != "no_alo_whi":
                        acc = acc + al @ bh
                    if fault != "no_wlo_ahi":
                        acc = acc + ah @ bl
                    acc = acc + ah @ bh
        acc = acc.view(s.imgs, s.H, s.W, s.N).permute(0, 3, 1, 2)
        resp = res if k else o.resp
        if fault == "resid_cb" and resp is not None:
            resp = torch.roll(resp, -2, 1)                                       # 32 columns = two records further
        out = epilogue(acc, asc, o.alpha if last else None, o.beta if last else None, resp, s.relu and last, s.f32 and last)
        res = None if last else pack_planes(out)
    return out
