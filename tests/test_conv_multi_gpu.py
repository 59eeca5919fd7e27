"""`sdf_spike_conv2d_multi_fwd`: the four output-parity classes of MS_SpikingTransposeDecoderLayer's ConvTranspose2d(k 3, s 2, p 1, op 1)
(reference Spiking_modules.py:461-474) as ONE launch of the streaming kernel - bit-equal to the four single launches (same kernel body,
same work items per class), and equal to torch's transposed convolution of the same spikes in fp64 to the two-plane weight precision."""
import pytest
import torch

from sdformerflow_amd import hip
from sdformerflow_amd.engine import deconv_classes
from sdformerflow_amd.synthetic import synth_uniform as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PP, REDUCE, MULTI = "spike_mm_pp_kernel<2, 0, true>", "splitk_reduce_kernel", "spike_mm_pp_multi_kernel<2>"
# What `sdf_spike_conv2d_multi_fwd` launches per shape: (kernel, workgroups) in order (csrc/spike_mm_pp.hip: tiles of 256 rows x 96 columns,
# K stages of 64; a class with at most 128 tiles and S >= 4 stages splits K, and then the library launches one by one).
LAUNCHES = {
    # M = 69 120: 270 tiles a class, no split-K; 270 items in pairs = 135 workgroups a class: ONE launch of 540
    (10, 72, 96, 196, 96): [(MULTI, 540)],
    # M = 252, 2 tiles a class, K = 48 .. 192 (S <= 3: no split-K): 2 workgroups a class: ONE launch of 8
    (4, 9, 7, 48, 192): [(MULTI, 8)],
    # M = 1920: 8 tiles; 112 channels, K = 112 | 224 | 224 | 448, S = 2 | 4 | 4 | 7: three of the classes split K -> one by one:
    # no split, 8 items | 2 chunks: 16 items in pairs | the same | 3 chunks: 24 items in pairs; reduce: 1920 * 24 quads / 256 = 180
    (10, 12, 16, 100, 96): [(PP, 8), (PP, 8), (REDUCE, 180), (PP, 8), (REDUCE, 180), (PP, 12), (REDUCE, 180)],
    # M = 252: 2 tiles; K = 64 | 128 | 128 | 256, S = 1 | 2 | 2 | 4: the 2 x 2 class splits K (2 chunks) -> one by one; 252 * 48 quads / 256 -> 48
    (4, 9, 7, 64, 192): [(PP, 2), (PP, 2), (PP, 2), (PP, 4), (REDUCE, 48)],
}
# under SDF_CONV_MULTI=0 the two shapes of the multi launch run their classes as four launches
ONE_BY_ONE = {(10, 72, 96, 196, 96): [(PP, 135)] * 4, (4, 9, 7, 48, 192): [(PP, 2)] * 4}


def _assert_launches(log, want):
    assert len(log.rows) == len(want), (log.rows, want)
    for (name, wgs, *_), (kernel, wwgs) in zip(log.rows, want):
        mangled = kernel.replace("<2, 0, true>", "ILi2ELi0ELb1EE").replace("<2>", "ILi2EE")
        assert (kernel in name or mangled in name) and wgs == wwgs, (name, wgs, kernel, wwgs)


@pytest.mark.parametrize("imgs,H,W,Cin,Cout", [(10, 72, 96, 196, 96), (10, 12, 16, 100, 96), (4, 9, 7, 64, 192), (4, 9, 7, 48, 192)])
def test_parity_classes_in_one_launch(imgs, H, W, Cin, Cout, monkeypatch):
    cp = (Cin + 15) // 16 * 16
    s = torch.zeros((imgs, H, W, cp), dtype=torch.uint8)
    s[..., :Cin] = (rnd((imgs, H, W, Cin), 500) < 0.3).to(torch.uint8)
    w = rnd((Cin, Cout, 3, 3), 501, -0.08, 0.08)
    alpha, beta = rnd((Cout,), 502, 0.5, 1.5).to(DEV), rnd((Cout,), 503, -0.2, 0.2).to(DEV)
    classes = deconv_classes(w.to(DEV), imgs, H, W, cp, 2, DEV)
    sd = s.to(DEV)

    def run(multi, want=None):
        z = torch.full((imgs, 4 * H * W, Cout), float("nan"), device=DEV)
        if multi:
            with hip.launch_log() as log:
                hip.spike_conv2d_multi(sd, classes, imgs, H, W, cp, H, W, z, alpha=alpha, beta=beta)
            if want is not None:
                _assert_launches(log, want)
        else:
            for c in classes:
                hip.spike_conv2d(sd, c["Wp"], imgs, H, W, cp, H, W, c["KH"], c["KW"], 1, c["dy"], c["dx"], out=z, alpha=alpha, beta=beta,
                                 out_rowmap=c["rowmap"])
        torch.cuda.synchronize()
        return z
    want = LAUNCHES[(imgs, H, W, Cin, Cout)]
    one, four = run(True, want), run(False)
    assert torch.equal(one, four) and not torch.isnan(one).any()
    monkeypatch.setenv("SDF_CONV_MULTI", "0")                   # the entry point's own one-by-one path
    single = ONE_BY_ONE.get((imgs, H, W, Cin, Cout), want)      # (the fallback IS the one-by-one path)
    assert torch.equal(run(True, single), four)
    ref = torch.nn.functional.conv_transpose2d(s[..., :Cin].permute(0, 3, 1, 2).double(), w.double(), None, 2, 1, 1)
    ref = ref.permute(0, 2, 3, 1) * alpha.cpu().double() + beta.cpu().double()
    err = (one.cpu().view(imgs, 2 * H, 2 * W, Cout).double() - ref).abs().max().item()
    assert err <= 2e-5 * ref.abs().max().item(), err


@pytest.mark.parametrize("imgs,T,H,W,Cin,Cout", [(10, 10, 72, 96, 196, 48), (10, 10, 21, 37, 196, 48), (10, 10, 12, 16, 100, 96), (20, 10, 9, 7, 64, 48), (20, 20, 5, 6, 196, 48),
                                                  (10, 10, 1, 1, 48, 8), (10, 10, 7, 1, 250, 24)])
def test_transposed_convolution_as_one_product(imgs, T, H, W, Cin, Cout, monkeypatch):
    """`sdf_spike_deconv3x3s2_fwd` (round 5): the same ConvTranspose2d(3, 2, 1, 1) + BatchNorm as ONE digit product - a row is an input
    pixel, its K the 2 x 2 input neighbourhood (zero beyond the image: the last row / column, and every neighbour of a 1 x 1 image), its
    4 Cout columns the 2 x 2 output block.  Within 1e-5 of fp64 on the output's magnitude (23-bit digits, exact integer sums) and of the
    parity-class launches; every output element written (NaN pre-fill)."""
    cp = (Cin + 15) // 16 * 16
    s = torch.zeros((imgs, H, W, cp), dtype=torch.uint8)
    s[..., :Cin] = (rnd((imgs, H, W, Cin), 510 + H) < 0.3).to(torch.uint8)
    w = rnd((Cin, Cout, 3, 3), 511, -0.08, 0.08)
    alpha, beta = rnd((Cout,), 512, 0.5, 1.5).to(DEV), rnd((Cout,), 513, -0.2, 0.2).to(DEV)
    assert hip.deconv2x2_applicable(imgs, T, H, W, cp, Cout)
    planes = hip.pack_deconv2x2_weight(w.to(DEV), cp)
    z = torch.full((imgs, 2 * H, 2 * W, Cout), float("nan"), device=DEV)
    hip.spike_deconv3x3s2(s.to(DEV), planes, imgs, T, H, W, cp, Cout, alpha=alpha, beta=beta, out=z)
    torch.cuda.synchronize()
    ref = torch.nn.functional.conv_transpose2d(s[..., :Cin].permute(0, 3, 1, 2).double(), w.double(), None, 2, 1, 1)
    ref = ref.permute(0, 2, 3, 1) * alpha.cpu().double() + beta.cpu().double()
    got = z.cpu().double()
    assert not torch.isnan(got).any()
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    # bit-equal to itself run to run (exact integer sums), and - on weights both formats hold exactly - to the parity-class launches
    z2 = torch.empty_like(z)
    hip.spike_deconv3x3s2(s.to(DEV), planes, imgs, T, H, W, cp, Cout, alpha=alpha, beta=beta, out=z2)
    assert torch.equal(z, z2)
    # the halo-tile kernel (208 padded channels, >= 4 096 pixels) and the row-loop kernel's form of the product: the same exact sums
    monkeypatch.setenv("SDF_DECONV_WRES", "0")
    z3 = torch.full_like(z, float("nan"))
    hip.spike_deconv3x3s2(s.to(DEV), planes, imgs, T, H, W, cp, Cout, alpha=alpha, beta=beta, out=z3)
    monkeypatch.delenv("SDF_DECONV_WRES")
    assert torch.equal(z, z3)
    if Cout % 96 == 0:
        wq = (w * 1024).round() / 1024
        zq = hip.spike_deconv3x3s2(s.to(DEV), hip.pack_deconv2x2_weight(wq.to(DEV), cp), imgs, T, H, W, cp, Cout)
        zc = torch.full((imgs, 4 * H * W, Cout), float("nan"), device=DEV)
        hip.spike_conv2d_multi(s.to(DEV), deconv_classes(wq.to(DEV), imgs, H, W, cp, 2, DEV), imgs, H, W, cp, H, W, zc)
        assert torch.equal(zq.view(imgs, 4 * H * W, Cout), zc)
