"""Linear layer on two fp16 planes per operand (csrc/dense_linear.hip) against torch's fp64 matmul: the qkv / proj / fc1 / fc2
projections of the ANN swin block (reference models/STSwinNet/swin_transformer3D_v2.py:15-34, 176-202, 272-313) with bias, GELU
and the shortcut add in the epilogue."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = [
    # M, K, N, bias, gelu, resid
    (1000, 96, 288, True, False, False),        # qkv, ragged last row tile
    (4096, 96, 96, True, False, True),          # proj + shortcut
    (777, 96, 384, True, True, False),          # fc1 + GELU
    (2048, 384, 96, True, False, True),         # fc2 + shortcut
    (640, 1536, 384, False, False, False),      # stage-2 fc2 shape, no bias
    (128, 32, 96, True, True, True),            # one tile, one k chunk
]


@pytest.mark.parametrize("M,K,N,bias,gelu,res", CASES)
def test_dense_linear_matches_fp64(M, K, N, bias, gelu, res):
    from sdformerflow_amd import hip
    g = torch.Generator().manual_seed(M + K + N)
    a = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda() if bias else None
    r = torch.randn(M, N, generator=g).cuda() if res else None
    assert hip.dense_linear_applicable(M, N, K)
    y = hip.dense_linear(a, hip.pack_dense_linear_weight(w), b, gelu, r)
    ref = a.double().cpu() @ w.double().cpu().T
    if bias:
        ref = ref + b.double().cpu()
    if gelu:
        ref = F.gelu(ref)
    if res:
        ref = ref + r.double().cpu()
    err = (y.double().cpu() - ref).abs().max().item()
    assert err <= 4e-6 * ref.abs().max().item(), (err, ref.abs().max().item())


def test_in_place_shortcut_and_rejections():
    from sdformerflow_amd import hip
    g = torch.Generator().manual_seed(3)
    a = torch.randn(300, 96, generator=g).cuda()
    w = (torch.randn(96, 96, generator=g) / 10).cuda()
    x = torch.randn(300, 96, generator=g).cuda()
    ref = x + F.linear(a, w)
    out = hip.dense_linear(a, hip.pack_dense_linear_weight(w), None, False, x, out=x)       # x += a @ w.T
    assert out.data_ptr() == x.data_ptr()
    assert (x - ref).abs().max().item() <= 1e-5
    with pytest.raises(hip.SdfError):
        hip.dense_linear(a, hip.pack_dense_linear_weight(torch.randn(64, 96).cuda()))          # N % 96
    with pytest.raises(hip.SdfError):
        hip.dense_linear(torch.randn(10, 48).cuda(), hip.pack_dense_linear_weight(torch.randn(96, 48).cuda()))   # K % 32


@pytest.mark.parametrize("rows,C", [(1000, 96), (333, 192), (100, 384), (64, 768), (17, 1536), (5, 100), (9, 2048)])
def test_layer_norm_matches_torch(rows, C):
    """sdf_layer_norm_fwd against nn.LayerNorm in fp64 (reference swin_transformer3D_v2.py: norm1 / norm2 / PatchMerging.norm / norm{i})."""
    from sdformerflow_amd import hip
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 3 + 1.5).cuda()
    w, b = (0.5 + torch.rand(C, generator=g)).cuda(), torch.randn(C, generator=g).cuda()
    y = hip.layer_norm(x, w, b, 1e-5)
    ref = F.layer_norm(x.double().cpu(), (C,), w.double().cpu(), b.double().cpu(), 1e-5)
    assert (y.double().cpu() - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()


@pytest.mark.parametrize("imgs,H,W,C,N,stride,T", [(4, 24, 32, 96, 96, 4, 2), (2, 17, 21, 32, 192, 2, 0), (6, 12, 12, 64, 96, 1, 3)])
def test_strided_convolution_as_gathered_gemm(imgs, H, W, C, N, stride, T):
    """The convolution form of sdf_dense_linear_fwd (PatchEmbedLocal.proj, reference models/STSwinNet/PatchEmbed.py:191) against
    F.conv2d in fp64, including the (T, B) -> (B, T) image order of the output."""
    from sdformerflow_amd import hip
    g = torch.Generator().manual_seed(imgs * H + C)
    x = torch.randn(imgs, C, H, W, generator=g).cuda()
    w = (torch.randn(N, C, 3, 3, generator=g) / (3 * C ** 0.5)).cuda()
    b = torch.randn(N, generator=g).cuda()
    wp = hip.pack_dense_linear_weight(w.permute(0, 2, 3, 1).reshape(N, -1))
    y = hip.dense_conv3x3_strided(x.permute(0, 2, 3, 1).contiguous(), wp, b, stride, T)
    ref = F.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), stride, 1).permute(0, 2, 3, 1)
    if T:
        ref = ref.reshape(T, imgs // T, *ref.shape[1:]).transpose(0, 1).reshape(ref.shape)
    assert y.shape == ref.shape
    err = (y.double().cpu() - ref).abs().max().item()
    assert err <= 4e-6 * ref.abs().max().item(), (err, ref.abs().max().item())


@pytest.mark.parametrize("M,K,N,bias", [c[:4] for c in CASES] + [(1, 96, 96, True), (129, 96, 288, True)])
def test_dense_linear_per_element_at_the_initial_weight_scale(M, K, N, bias):
    """Per element instead of per max |ref|: |y - ref64| <= 2e-6 (sum_k |a| |w| + |bias|) + 2^-25 sum_k |w|.  The first term is the
    bound of the project's fp32-accumulation tests (22-bit products, fp32 sums).  The second is the fp16 subnormal floor of the
    activation split: below 2^-14 fp16 has the fixed spacing 2^-24, so a_hi + a_lo misses a by up to 2^-25 absolute however small a is
    (the weights are pre-scaled by the packer and have no such floor).  Weights as swin initialises them (trunc-normal std 0.02, cut
    at +-0.04); the rows of a span 1e-7 ... 1e2, so whole rows have fp16-subnormal hi halves: a matrix pipe that flushed subnormal
    inputs would return 0 for them and miss this bound by orders of magnitude.  Plain product + bias (the epilogues are held by the
    tests above); the six shapes of CASES, a single row, and one row beyond a 128-row tile."""
    from sdformerflow_amd import hip
    g = torch.Generator().manual_seed(7 * M + K + N)
    a = torch.randn(M, K, generator=g) * 10.0 ** (-9.0 * torch.rand(M, 1, generator=g) + 2.0)
    w = (0.02 * torch.randn(N, K, generator=g)).clamp(-0.04, 0.04)
    b = 0.02 * (2 * torch.rand(N, generator=g) - 1) if bias else None
    assert hip.dense_linear_applicable(M, N, K)
    y = hip.dense_linear(a.cuda(), hip.pack_dense_linear_weight(w.cuda()), b.cuda() if bias else None).double().cpu()
    ref = a.double() @ w.double().T
    mag = a.double().abs() @ w.double().abs().T
    if bias:
        ref, mag = ref + b.double(), mag + b.double().abs()
    allow = 2e-6 * mag + 2.0 ** -25 * w.double().abs().sum(1)
    ratio = ((y - ref).abs() / allow)
    sub = (a.abs().max(1).values < 2.0 ** -14)                                    # rows whose every hi half is subnormal in fp16
    print(f"\nDENSEPAR {M}x{K}x{N} err/allowance {ratio.max().item():.3f}; rows with subnormal hi halves: {int(sub.sum())}, theirs "
          f"{ratio[sub].max().item() if sub.any() else 0.0:.3f}")
    assert bool((ratio <= 1.0).all()), ratio.max().item()
