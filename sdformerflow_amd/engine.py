"""HIP execution engine of the MS (membrane-shortcut) SDformerFlow family.

Turns the module tree (state_dict holder) into a flat schedule of C-ABI kernel launches:

  * weights of every spike-fed Linear are pre-split into bf16 planes (fp32-grade on the bf16 MFMA path)
  * eval-BatchNorm becomes (alpha, beta) vectors applied as one fmaf inside the producing / consuming kernel
  * pad + roll + window_partition_v2 (+ the raw .view) and window_reverse + roll + crop become one int32
    row map per (shape, shift), used as a gather by the neuron kernel and as a scatter by the GEMM epilogue
  * the residual adds of the block happen in the GEMM epilogues, in place, on the (B,D,H,W,C) activation
  * spikes travel as 1 byte between kernels
  * the convolutions either side of the swin stages (patch embedding, U-Net tail: SURVEY.md 8f rows 1-2) are implicit-GEMM
    spike convolutions with the BN / residual / neuron epilogues fused; the large 96-channel 3x3 launches take int8 digit
    planes and the weight-resident kernel (csrc/spike_conv_wres.hip); no library kernel is left in the SNN forward
  * `forward(x, replicas=True)`: the B samples are B independent batch-1 forwards in one launch sequence (round 6; the route functions, `_slice_map`)
  * `tape` (tests only) keeps every neuron layer's spikes for the spike-forced oracle replay (tests/replay.py); a firing-rate
    monitor (monitor.py) takes the same recording route and counts the spikes instead of keeping them - under replicas per sample
    (monitor.ReplicaFiringRateMonitor; `_rec` says where a record's samples lie), where the tape stays refused

Reference schedule being replaced: models/STSwinNet_SNN/Spiking_STSwinNet.py:161-182,278-305 and the
call tree of SURVEY.md 3.2.  No CPU fallback: everything here raises off-GPU.
"""
from __future__ import annotations

from collections import namedtuple
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import hip
from .STSwinNet_SNN.Spiking_swin_transformer3D import get_window_size, merge_row_map, window_slice_map

BN_EPS = 1e-5
# Narrowest stage that runs on int8 digit planes with the neurons in the producing kernels' epilogues: from C = 96 (swin stage 0) on
# since round 5 - stages 0 - 1 (C <= 192) on the weight-resident row-loop kernels of csrc/ms_res.hip, stages 2 - 3 on csrc/ms_wide.hip
# (round 4 had the wide kernels from C = 192 and qk_front / spike_gemm / ms_mlp_fused on the fp16 planes at stage 0).
_WIDE_MINC = 96


def bn_affine(bn, device):
    """(alpha, beta) of an eval BatchNorm, computed on the host exactly like ATen's CPU kernel:
    alpha = w * rsqrt(var + eps) (fp32), beta = fma(-mean, alpha, bias)."""
    w, b = bn.weight.detach().float().cpu(), bn.bias.detach().float().cpu()
    m, v = bn.running_mean.detach().float().cpu(), bn.running_var.detach().float().cpu()
    alpha = w * torch.rsqrt(v + BN_EPS)
    beta = (b.double() - m.double() * alpha.double()).float()
    return alpha.contiguous().to(device), beta.contiguous().to(device)


class _Lin:
    """A Linear fed by spikes: bf16 weight planes + optional bias + the BN that follows it."""

    def __init__(self, linear, bn, device, nsplit, digits=True):
        w = linear.weight.detach().float().to(device).contiguous()
        self.N, self.K = w.shape
        self.Wp = hip.split_weight(w, nsplit)
        # wide layers (swin stages 1 - 3) also carry int8 digit planes: what csrc/ms_wide.hip multiplies by (default plane mode only)
        # (`digits=False`: callers whose layer never reaches a digit kernel - the SEW family's fc2 - skip the extra 3 bytes per weight)
        self.digits = hip.split_weight_i8x3(w) if digits and nsplit == 2 and self.K >= _WIDE_MINC and self.K % 32 == 0 and self.N % 32 == 0 else None
        self.bias = None if linear.bias is None else linear.bias.detach().float().to(device).contiguous()
        self.alpha, self.beta = bn_affine(bn, device) if bn is not None else (None, None)


def _np(sn_module, device):
    """NeuronParams of a Spiking_neuron wrapper, PSN weights moved to the device."""
    n = sn_module.spiking_neuron
    if n.kind not in hip.KIND:
        raise hip.SdfError(f"neuron {type(n).__name__}: no fused kernel (lif / if / psn / plif / SLTTlif have one); it runs as a stand-alone "
                           "module (reference Spiking_modules.py:84-92), and a whole MS model in eval mode on the unfused plan "
                           "(model.eval_engine(): engine_glif.GLIFFlowEngine)")
    if n.kind == "psn":
        return hip.NeuronParams("psn", psn_w=n.weight.detach().float().to(device).contiguous(),
                                psn_b=n.bias.detach().float().reshape(-1).to(device).contiguous())
    return hip.NeuronParams(n.kind, n.tau, n.v_threshold, n.v_reset)


def attention_score(e, sn, nH, Tq, B_, N1, launch=None, rep=1):
    """`attn = self.attn_sn(x)` of `Spiking_QK_WindowAttention3D.forward` (reference Spiking_swin_transformer3D.py:709-711) from the
    gated spikes e (T', B_*N1, C) u8 of one block: the head scramble Z[t,b,n,g,d] = E_flat[((((b nH + g) T' + t) N1 + n) hd + d] as a
    re-layout (diagnostic path: the score is dead on the forward path, :715-716), then the neuron kernel over T' (`launch`: the
    engine's neuron launch).  -> (T', B_, N1, C) fp32 spikes.  `rep` > 1: the B_ windows are `rep` independent batch-1 problems
    (hip.replica_slice_map): every sample's E_flat is the sub-block [:, r * nW : (r + 1) * nW] and is scrambled on its own."""
    Cc, nW = e.shape[-1], B_ // rep
    z = e.reshape(Tq, rep, nW * N1 * Cc).transpose(0, 1).reshape(rep, nW, nH, Tq, N1, Cc // nH).permute(3, 0, 1, 4, 2, 5)
    z = z.reshape(Tq, B_ * N1 * Cc).float().contiguous()
    out = torch.empty_like(z)
    n = z.shape[1]
    (launch or hip.neuron_fwd)(z, out, Tq, 1, n, 0, n, 0, n, sn)
    return out.view(Tq, B_, N1, Cc)


class _Block:
    def __init__(self, blk, device, nsplit, name="", np=_np):
        self.name = name
        a = blk.attn
        self.attn_sn = np(a.attn_sn, device)
        self.nH, self.window_size, self.shift_size = a.num_heads, blk.window_size, blk.shift_size
        self.q = _Lin(a.linear_q, a.bn_q.norm_layer, device, nsplit)
        self.k = _Lin(a.linear_k, a.bn_k.norm_layer, device, nsplit)
        self.p = _Lin(a.proj, a.proj_bn.norm_layer, device, nsplit)
        self.pe = a.positional_encoding.detach().float().to(device).contiguous()
        self.sn_proj, self.sn_q, self.sn_k, self.sn2_q = (np(m, device) for m in (a.proj_sn, a.sn_q, a.sn_k, a.sn2_q))
        # q and k read the same spikes: with parameter-free neurons of equal settings (LIF / IF) they run as ONE fused GEMM
        # over the stacked weights [Wq; Wk]; the positional term only exists for the k half (q adds zeros)
        self.qk = None
        sq, sk = self.sn_q, self.sn_k
        if sq.kind in ("lif", "if") and (sq.kind, sq.tau, sq.v_th, sq.v_reset) == (sk.kind, sk.tau, sk.v_th, sk.v_reset):
            w = torch.cat([a.linear_q.weight.detach().float(), a.linear_k.weight.detach().float()], 0).to(device).contiguous()
            self.qk = {"Wp": hip.split_weight(w, nsplit), "digits": hip.split_weight_i8x3(w) if self.q.digits is not None else None,
                       "alpha": torch.cat([self.q.alpha, self.k.alpha]).contiguous(),
                       "beta": torch.cat([self.q.beta, self.k.beta]).contiguous(),
                       # the positional table is consumed as flat (Tq, N1, C) memory (the reference's raw reshape, :678-679)
                       "add": torch.cat([torch.zeros((self.pe.numel() // self.q.N, self.q.N), device=device),
                                         self.pe.reshape(-1, self.q.N)], -1).contiguous()}
        m = blk.mlp
        self.fc1 = _Lin(m.fc1, m.bn1.norm_layer, device, nsplit)
        self.fc2 = _Lin(m.fc2, m.bn2.norm_layer, device, nsplit)
        if self.fc2.digits is not None and self.fc2.K >= 1536:      # wide stages: fc2 (K = 4 C against few tokens) runs on the small-M kernel
            self.fc2.digits_tiled = hip.tile_weight_i8x3(self.fc2.digits)
        self.sn1, self.sn2 = np(m.sn1, device), np(m.sn2, device)


def _conv_planes(w, nsplit, cin_pad=None):
    return hip.pack_conv_weight(w.detach().float(), nsplit, cin_pad)


def _conv_digits(w, nsplit):
    """int8 digit planes of a 3x3 convolution: on 96 input channels what the weight-resident kernel reads for large launches
    (csrc/spike_conv_wres.hip), on multiples of 64 what the small-M kernel reads (csrc/ms_smallm.hip: the U-Net bottleneck); None where
    neither has an instantiation or the exact 3-plane / 1-plane modes were asked for."""
    if nsplit != 2 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] % 32 or not (w.shape[1] in (48, 96) or w.shape[1] % 64 == 0):
        return None
    return hip.pack_conv_weight_i8x3(w.detach().float(), tiled=w.shape[1] not in (48, 96))   # (fragment order: only the small-M kernel reads those)


class _ResBlock:
    """MS_ResBlock weights for the spike-convolution path (3x3, pad 1, NHWC)."""

    def __init__(self, rb, device, nsplit, name="", np=_np):
        self.name = name
        self.C = rb.conv1[0].weight.shape[0]
        self.w1, self.w2 = _conv_planes(rb.conv1[0].weight, nsplit), _conv_planes(rb.conv2[0].weight, nsplit)
        self.w1.digits, self.w2.digits = _conv_digits(rb.conv1[0].weight, nsplit), _conv_digits(rb.conv2[0].weight, nsplit)
        self.bn1, self.bn2 = bn_affine(rb.norm1.norm_layer, device), bn_affine(rb.norm2.norm_layer, device)
        self.sn1, self.sn2 = np(rb.sn1, device), np(rb.sn2, device)


_DECONV_ROWMAPS = {}


def deconv_classes(w, imgs, H, W, cin_pad, nsplit, device):
    """ConvTranspose2d(k=3, s=2, p=1, output_padding=1) as four output-parity classes.

    out[2y'+py, 2x'+px] only receives the taps whose kernel index has the right parity
    (oy = 2*iy - 1 + ky): py = 0 -> (ky=1, iy=y'); py = 1 -> (ky=2, iy=y') and (ky=0, iy=y'+1); same in x.
    Each class is a 1- or 2-tap implicit GEMM over the INPUT grid whose rows are scattered to the class's
    output pixels by an int32 row map.  w is the reference layout (Cin, Cout, 3, 3)."""
    Cin, Cout = w.shape[:2]
    taps = {0: [(0, 1)], 1: [(0, 2), (1, 0)]}            # parity -> [(input offset, kernel index)]
    out = []
    for py in (0, 1):
        for px in (0, 1):
            ty, tx = taps[py], taps[px]
            wk = torch.zeros((Cout, len(ty), len(tx), cin_pad), dtype=torch.float32, device=w.device)
            for a, (_, ky) in enumerate(ty):
                for b, (_, kx) in enumerate(tx):
                    wk[:, a, b, :Cin] = w.detach().float()[:, :, ky, kx].t()
            key = (imgs, H, W, py, px, str(device))
            if key not in _DECONV_ROWMAPS:
                i = torch.arange(imgs).view(-1, 1, 1)
                y = torch.arange(H).view(1, -1, 1)
                x = torch.arange(W).view(1, 1, -1)
                rm = ((i * 2 * H + 2 * y + py) * 2 * W + 2 * x + px).reshape(-1).to(torch.int32)
                _DECONV_ROWMAPS[key] = rm.to(device)
            out.append({"Wp": hip.split_weight(wk.reshape(Cout, -1), nsplit), "KH": len(ty), "KW": len(tx),
                        "dy": [t[0] for t in ty], "dx": [t[0] for t in tx], "rowmap": _DECONV_ROWMAPS[key]})
    return out


def _pad16(c):
    return (c + 15) // 16 * 16


def _pad32(c):
    return (c + 31) // 32 * 32


def deconv_tap_weights(w, cin_pad, nsplit):
    """ConvTranspose2d weight (Cin, Cout, 3, 3) -> planes of the stacked per-tap matrices (9*Cout, cin_pad): row
    (ky*3+kx)*Cout + co holds w[:, co, ky, kx] (zero for padded input channels)."""
    Cin, Cout = w.shape[:2]
    wk = torch.zeros((9 * Cout, cin_pad), dtype=torch.float32, device=w.device)
    wk[:, :Cin] = w.detach().float().permute(2, 3, 1, 0).reshape(9 * Cout, Cin)
    planes = hip.split_weight(wk, nsplit)
    form = _tap_digits(nsplit, cin_pad)
    if form == "tiled":
        planes.digits = hip.tile_weight_i8x3(hip.split_weight_i8x3(wk))
    elif form == "rm":
        planes.digits_rm = hip.split_weight_i8x3(wk)
    return planes


def _tap_digits(nsplit, cin_pad):
    """The int8 digit form the stacked tap matrix of a decoder also has: "tiled" (fragment order: the small-M kernel's operand),
    "rm" (row-major: the weight-resident row-loop kernel, csrc/ms_res.hip) or None (16-bit planes only)."""
    if nsplit != 2 or cin_pad % 16:
        return None
    if cin_pad % 64 == 0 and cin_pad >= 1024:
        return "tiled"
    return "rm" if cin_pad <= 1024 else None


def _center_pad(p, h, w):
    """(B,D,h',w',C) centred in (h, w) (cropped where larger): the reference's skip_concat alignment."""
    dh, dw = h - p.shape[2], w - p.shape[3]
    return F.pad(p, (0, 0, dw // 2, dw - dw // 2, dh // 2, dh - dh // 2))


def _pred_planes(conv, device, nsplit):
    """Flow prediction = 1x1 convolution with 2 output channels on spikes: the spike GEMM with the weight rows padded to one 32-column
    block (columns 2.. are zero and never read back).  -> (planes, bias (32), the (2, Cin) weight itself)"""
    w2 = conv.weight.detach().float().reshape(conv.weight.shape[0], -1)
    wp = torch.zeros((32, w2.shape[1]), dtype=torch.float32, device=device)
    wp[:w2.shape[0]] = w2
    bp = torch.zeros(32, dtype=torch.float32, device=device)
    bp[:w2.shape[0]] = conv.bias.detach().float()
    return hip.split_weight(wp, nsplit), bp, w2


# A decoder level: ConvTranspose2d weight (Cin, Cout, 3, 3) in the reference's channel order, the BN behind it, the neuron in front.
_Decoder = namedtuple("_Decoder", "w bn sn")
# A prediction head: the padded GEMM form (planes, bias, nout of its 32 columns) and, in the MS family, its neuron with the (nout, Cin)
# weight and the bias the one-launch head kernel reads.
_Pred = namedtuple("_Pred", "planes bias nout sn w b", defaults=(None, None, None))


# ------------------------------------------------------------------ routes
# Which kernel serves a layer, and how many samples go into one launch, is decided HERE - by pure functions of shapes and flags (no
# tensors: they answer on a machine without a GPU, tests/test_engine_routes_cpu.py) - and nowhere else; the methods below ask, allocate
# and launch.  Two rules are stated in these functions only:
#   replicas: every layer takes the kernel family and weight representation of its batch-1 forward, whatever the
#     size rules say about B-fold rows - else the flows are not the batch-1 flows bit for bit - in the largest sample chunk per launch
#     that is still routed like ONE sample;
#   31-bit operand offsets: a launch too large for them goes in equal chunks of whole samples (batch elements are independent).
def _largest_divisor(B, ok):
    """Largest n among the DIVISORS of B with ok(n), 0: none.  Divisors, so that every chunk is the same launch: a ragged last chunk
    could miss a kernel's "enough tiles" rule and fall to a streaming kernel that has no T = 5 / 20 form."""
    return next((n for n in range(B, 0, -1) if B % n == 0 and ok(n)), 0)


class ConvRoute(NamedTuple):
    form: str           # "smallm" | "wres" | "wres_neuron" | "stream": the `_conv_<form>` launch helper of the engine
    samples: int        # batch elements per launch (a divisor of B)


def conv3x3_route(B, D, h, w, Cin, Cout, stride, digits, kind=None, replicas=False):
    """Kernel form of a 3x3 / pad 1 spike convolution on (B,D,h,w,Cin) and the samples per launch.  `digits`: the layer has int8 digit
    planes beside its 16-bit planes; `kind`: the neuron the caller hands over (None: fp32 output)."""
    if not digits:
        # 16-bit planes only: the streaming kernels' tile family and split-K plan follow the row count - replicas go sample by sample
        return ConvRoute("stream", 1 if replicas else B)

    def asked(n):           # what the size rules say about n samples in one launch
        return (hip.smallm_conv_applicable(n * D, h, w, Cin, Cout, stride, D), hip.conv_wres_applicable(n * D, h, w, Cin, Cout, stride, 1),
                hip.conv_wres_applicable(n * D, h, w, Cin, Cout, stride, D))
    n = B
    if replicas and B > 1:
        one = asked(1)
        n = _largest_divisor(B, lambda m: asked(m) == one)
    if n > 1 and not hip.conv_wres_applicable(n * D, h, w, Cin, Cout, stride, 1):
        # too large for the digit kernel's 31-bit operand offsets as one launch (configs[4]: 80 images of 240 x 320 x 96 fp32)
        n = _largest_divisor(n, lambda m: hip.conv_wres_applicable(m * D, h, w, Cin, Cout, stride, 1)) or n
    smallm, wres, wres_fused = asked(n)
    if smallm and kind in (None, "lif", "if", "psn"):
        # few rows against many weights (the U-Net bottleneck: 1 080 rows x 768 x 6 912): one launch, K split over the waves of a
        # workgroup, sum + BN + shortcut + neuron in its epilogue (csrc/ms_smallm.hip)
        return ConvRoute("smallm", n)
    # wres: large launches on 96 channels - int8 digit planes, weights resident in LDS (csrc/spike_conv_wres.hip); else the streaming
    # kernels on the 16-bit planes, fused or fp32
    if kind is None:
        return ConvRoute("wres" if wres else "stream", n)
    if kind == "psn" or D not in (5, 10, 20):
        # the digit kernel's fused form is LIF / IF over T = 5 / 10 / 20; other neurons (the shipped PSN) take its fp32 form and
        # the neuron kernel behind it - still ahead of the streaming kernel's fused epilogue (profiles/r2j_psn.txt)
        return ConvRoute("wres_neuron" if wres else "stream", n)
    return ConvRoute("wres" if wres_fused else "stream", n)


def conv3x3_carries_neuron(B, D, h, w, Cin, Cout, stride, digits, kind, replicas=False):
    """Whether the caller of a 3x3 convolution hands the neuron behind it to `_conv3x3` (else: the bare fp32 convolution, whose epilogue
    can split K over the chip, then BN + neuron as one launch of their own).  The fused-neuron epilogue pays off once the tiles fill the
    chip.  The streaming kernels have it for T = 10; the weight-resident digit kernel rolls its time loop and takes T = 5 / 20 as well
    (configs[4]), at stride 2 (the patch embedding's first 3x3) as at stride 1; the small-M kernel always carries its neuron."""
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    big = ((1 if replicas else B) * D * oh * ow + 255) // 256 * (Cout // 96) >= 128
    if big and D == 10:
        return True
    if conv3x3_route(B, D, h, w, Cin, Cout, stride, digits, kind, replicas).form == "smallm":
        return True
    return big and conv3x3_route(B, D, h, w, Cin, Cout, stride, digits, "lif", replicas).form == "wres"


class DeconvRoute(NamedTuple):
    form: str           # "taps_smallm" | "taps_res" | "taps_stream" | "one_product" | "classes_multi" | "classes_each"
    cp: int             # padded channel count of the level's NHWC spike image
    images: int         # images (sample x time step) per launch


class _Level(NamedTuple):
    """A decoder level as `unet_tail` plans it.  `same`: the level's input y has the skip tensor's size, so its spike image is assembled
    without a concatenation, in the physical channel order [y | skip | prediction padded to 4]; else the reference's concatenation
    [prediction | y | skip] is made.  `cin`: channels of that image before padding."""
    same: bool
    cin: int
    route: DeconvRoute


def deconv_route(B, D, h, w, cin, cout, nsplit, replicas=False):
    """Route of a decoder's ConvTranspose2d(k 3, s 2, p 1, op 1) on (B,D,h,w,cin) spikes, the padded channel count of its spike image and
    the images per launch."""
    one, rows, imgs = (1 if replicas else B), D * h * w, B * D
    if one * rows * 9 * cout * 4 <= 64 << 20:
        # small levels: ONE plain spike GEMM over the nine stacked tap matrices + a col2im pass fills the chip; the four parity-class
        # convolutions (no 9x intermediate) are kept where that intermediate would cost more than it saves
        cp = _pad32(cin)
        form = _tap_digits(nsplit, cp)
        if form == "tiled" and hip.smallm_gemm_applicable(one * rows, 9 * cout, cp):
            # few rows against many weights (level 0: 1 080 x 3 456 x 1 536): csrc/ms_smallm.hip
            return DeconvRoute("taps_smallm", cp, D * _largest_divisor(B, lambda n: hip.smallm_gemm_rows_ok(n * rows)))
        if form == "rm" and hip.res_gemm_applicable(one * rows, 9 * cout, cp):
            # the middle levels (4 320 x 1 728 x 800, 17 280 x 864 x 416): csrc/ms_res.hip
            return DeconvRoute("taps_res", cp, D * _largest_divisor(B, lambda n: hip.res_gemm_applicable(n * rows, 9 * cout, cp)))
        return DeconvRoute("taps_stream", cp, D * one)      # (16-bit planes: the streaming kernels' split-K plan follows the row count)
    cp = _pad16(cin)
    # the conv kernels address their operands with 31-bit byte offsets: a larger z (config 5: 80 images of 240 x 320 x 96 fp32) goes
    # image chunk by image chunk - whole batch elements in equal chunks where that fits
    fits = lambda n: n * 4 * h * w * cout * 4 < 1 << 31
    per = D * (_largest_divisor(B, lambda n: fits(n * D)) or B)
    while not fits(per):
        per = (per + 1) // 2
    if nsplit == 2 and per % D == 0 and imgs % per == 0 and hip.deconv2x2_applicable(per, D, h, w, cp, cout, fast_only=True):
        # the last level: the transposed convolution as ONE digit product over the 2 x 2 input neighbourhood (a row = an input pixel,
        # its 4 cout columns = the 2 x 2 output block; halo tiles in LDS, weights resident: csrc/spike_deconv_wres.hip) instead of
        # four parity-class convolutions
        return DeconvRoute("one_product", cp, per)
    if replicas and B > 1:
        # the parity classes run on the streaming kernels (16-bit planes: tile family and split-K plan follow the row count): every
        # sample goes through the launches of its batch-1 forward
        return DeconvRoute("classes_multi", cp, D)
    # the four parity classes write disjoint rows of z and each fills about half of the chip: one launch for all of them where z fits
    return DeconvRoute("classes_multi" if per == imgs else "classes_each", cp, per)


class MSFlowEngine:
    _np = staticmethod(_np)         # how a Spiking_neuron wrapper is packed (engine_glif.GLIFFlowEngine packs gate tables)
    # the general neuron launch of every method below (engine_unfused.UnfusedFlowEngine's also keeps the membrane for a monitor)
    @staticmethod
    def _neuron_fwd(*a, **kw):
        return hip.neuron_fwd(*a, **kw)

    @classmethod
    def bare(cls, device, nsplit=2):
        """An engine without a model: the helpers (index maps, kernels, tape) for module-level `forward()` calls - the
        block-level classes of the module tree pack themselves and run through the same methods the model does."""
        e = cls.__new__(cls)
        if torch.device(device).type != "cuda":
            raise hip.SdfError("module forwards run on the MI355X HIP engine only (no CPU fallback): move the module and its input to 'cuda'")
        hip.lib()
        e.device, e.nsplit, e._maps, e._deconv, e.tape, e._masks, e.scores = torch.device(device), nsplit, {}, {}, None, {}, None
        e.replicas = False
        return e

    def __init__(self, model):
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise hip.SdfError("the SDformerFlow forward runs on the MI355X HIP engine only: call model.to('cuda') "
                               "(there is no CPU fallback; the CPU restatement lives in oracle/ for tests)")
        hip.lib()
        dev, ns = self.device, model.gemm_nsplit
        self.nsplit = ns
        unet = model.sttmultires_unet
        sw = unet.encoders.swin3d
        pe = sw.patch_embed
        self.num_bins, self.num_steps = pe.num_bins, pe.num_steps
        self.head_w = pe.head.conv[0].weight.detach().contiguous(memory_format=torch.channels_last)
        self.head_w_oihw = pe.head.conv[0].weight.detach().float().contiguous()
        self.head_bn, self.head_sn = bn_affine(pe.head.norm_layer.norm_layer, dev), self._np(pe.head.sn, dev)
        self.conv_w, self.conv_bn = _conv_planes(pe.conv.conv[0].weight, ns), bn_affine(pe.conv.norm_layer.norm_layer, dev)
        self.conv_w.digits = _conv_digits(pe.conv.conv[0].weight, ns)      # 48 -> 96 at stride 2: the digit kernel's even / odd halo form
        U = "sttmultires_unet."
        self.pe_name = U + "encoders.swin3d.patch_embed."
        self.pe_res = [_ResBlock(rb, dev, ns, self.pe_name + f"residual_encoding.resblocks.{i}.", self._np) for i, rb in enumerate(pe.residual_encoding.resblocks)]
        self.proj_res_w = pe.proj.conv_res.weight.detach().contiguous(memory_format=torch.channels_last)
        self.proj_res_w2 = pe.proj.conv_res.weight.detach().float().reshape(pe.proj.conv_res.weight.shape[0], -1).contiguous()
        self.proj_res_b = None if pe.proj.conv_res.bias is None else pe.proj.conv_res.bias.detach().float().contiguous()
        self.proj_w = _conv_planes(pe.proj.conv.weight, ns)
        self.proj_w.digits = _conv_digits(pe.proj.conv.weight, ns)         # 96 -> C at stride 2: the digit kernel's two-channel-pass form
        self.proj_bn, self.proj_sn = bn_affine(pe.proj.norm_layer, dev), self._np(pe.proj.sn, dev)
        self._maps, self._deconv = {}, {}
        self.tape = None            # parity tests set a list: every neuron layer's spikes are recorded (see _rec)
        self.scores = None          # `log=True`: a list that receives the attention score of the last block of every stage
        self.replicas = False       # forward(..., replicas=True): the batch is B independent batch-1 forwards (see forward)
        self._init_stages(model, unet, sw, dev, ns, U)

    def _init_stages(self, model, unet, sw, dev, ns, U):
        """Everything behind the patch embedding (the SEW engine packs its own: engine_sew.SEWFlowEngine)."""
        self.stages, self.merges = [], []
        for li, layer in enumerate(sw.layers):
            self.stages.append([_Block(b, dev, ns, U + f"encoders.swin3d.layers.{li}.swin_blocks.{bi}.", self._np) for bi, b in enumerate(layer.swin_blocks)])
            if layer.downsample is not None:
                d = layer.downsample
                self.merges.append((_Lin(d.reduction, d.norm.norm_layer, dev, ns), self._np(d.sn, dev)))
        self.unet_res = [_ResBlock(rb, dev, ns, U + f"resblocks.{i}.", self._np) for i, rb in enumerate(unet.resblocks)]
        self.decoders = [_Decoder(d.deconv[0].weight.detach(), bn_affine(d.norm_layer.norm_layer, dev), self._np(d.sn, dev)) for d in unet.decoders]
        self.preds = []
        for p in unet.preds:
            planes, bp, w2 = _pred_planes(p.conv[0], dev, ns)
            self.preds.append(_Pred(planes, bp, w2.shape[0], self._np(p.sn, dev), w2.to(dev).contiguous(), p.conv[0].bias.detach().float().to(dev).contiguous()))

    # ------------------------------------------------------------------ helpers
    def _slice_map(self, B, D, H, W, ws, ss):
        key = ("win", B, D, H, W, ws, ss, self.replicas)
        if key not in self._maps:
            if self.replicas and B > 1:
                # B independent batch-1 problems in one launch sequence: every sample keeps ITS batch-1 window view (hip.replica_slice_map)
                m1, nW = self._slice_map_1(D, H, W, ws, ss)
                if nW % ws[0]:
                    # (the head scramble of a sample must stay on one side of its attention-step boundary: hip.replica_zsrc_map, zg_rep)
                    raise hip.ReplicaGeometryError(f"replicas need a window count per sample ({nW}) that is a multiple of the window depth ({ws[0]})")
                self._maps[key] = (hip.replica_slice_map(m1, nW, B, ws[0], ws[1] * ws[2], D * H * W), B * nW)
            else:
                self._maps[key] = hip.window_slice_map(B, D, H, W, ws, ss, self.device)    # built on the device, cached per shape
        return self._maps[key]

    def _slice_map_1(self, D, H, W, ws, ss):
        key = ("win", 1, D, H, W, ws, ss, False)
        if key not in self._maps:
            self._maps[key] = hip.window_slice_map(1, D, H, W, ws, ss, self.device)
        return self._maps[key]

    def _merge_map(self, B, D, H, W):
        key = ("merge", B, D, H, W)
        if key not in self._maps:
            src, H2, W2 = merge_row_map(B, D, H, W)
            out_map = None
            if B > 1:       # GEMM rows are (t,b,h2,w2); the activation is laid out (b,t,h2,w2)
                t = torch.arange(D).view(D, 1, 1)
                b = torch.arange(B).view(1, B, 1)
                p = torch.arange(H2 * W2).view(1, 1, -1)
                out_map = ((b * D + t) * (H2 * W2) + p).reshape(-1).to(torch.int32).to(self.device)
            self._maps[key] = (torch.from_numpy(src.reshape(-1)).to(self.device), H2, W2, out_map)
        return self._maps[key]

    @staticmethod
    def _check_cl(x):
        """The kernels address activations as dense channel-last (B,D,h,w,C) fp32 buffers (and update them in place)."""
        if x.dim() != 5 or not x.is_contiguous() or x.dtype != torch.float32:
            raise hip.SdfError(f"expected a contiguous fp32 (B,D,h,w,C) tensor, got shape {tuple(x.shape)} strides {x.stride()} "
                               f"{x.dtype}; call .contiguous() (the update is in place)")

    # A firing-rate monitor (monitor.FiringRateMonitor / ReplicaFiringRateMonitor) while one of its forwards runs, else None: the
    # monitor's forward sets and clears it.
    monitor = None

    @property
    def taped(self):
        """Whether this forward takes the recording route - the kernels that leave every neuron layer's spikes in memory (bit-equal
        to the plain route, tests/test_replay_gpu.py): the parity tape or a firing-rate monitor asks for it.  Every site that
        chooses between the two routes asks HERE."""
        return self.tape is not None or self.monitor is not None

    def _rec(self, name, spikes, layout, steps=None):
        """The u8 spikes of neuron layer `name` (the state_dict prefix of its Spiking_neuron) on the recording route; `layout` says how
        they map onto the reference's tensor at that call: "flat" = same memory order (reshape; the time steps are the leading
        blocks - dim 0, or `steps` of them where the record is a (steps * rows, C) matrix), "BDHWC->TBCHW" / "BDHWC->TBHWC" =
        permute (time steps on dim 1).  The parity tape (tests only; `self.tape = []` switches it on, never during graph capture)
        keeps a copy; a firing-rate monitor counts them where they lie and keeps nothing.  Under replicas the record holds
        `_rec_samples` samples and the layout says on which side of the time axis they lie: "flat" = INSIDE (the samples are that many
        equal consecutive pieces of every time block: replica_slice_map puts sample r's windows at [r * nW, (r + 1) * nW) of every
        attention step, and the merge's rows are (t, b, h2, w2)), "BDHWC->..." = OUTSIDE (dim 0)."""
        if self.tape is not None:
            self.tape.append((name, spikes.clone(), layout))
        if self.monitor is not None:
            self._to_monitor(name, spikes if steps is None else spikes.view(steps, -1, spikes.shape[-1]), layout)

    _rec_samples = 1        # samples a record holds: the batch of forward(x, replicas=True) while it runs, else 1

    def _to_monitor(self, name, spikes, layout):
        # (only monitor.ReplicaFiringRateMonitor is let through to a replica forward: the others' record() takes no sample count)
        self.monitor.record(name, spikes, layout, **({"samples": self._rec_samples} if self._rec_samples > 1 else {}))

    def _rec_gates(self, blk, q, e, Tq, B_, N1):
        """Firing-rate monitor only: the two neuron calls of Spiking_QK_WindowAttention3D.forward whose spikes no kernel stores.
        `attn.sn2_q`, the token gate `self.sn2_q(q.sum(-1, keepdim=True))` on (T', B_, nH, N, 1) (reference :687-693), is RECOMPUTED
        here from the recorded q spikes - the head sums are exact small integers, the block's sn2_q runs over T' in the neuron kernel
        - and is not a read-out of the fused kernel's gate; that the two agree is what the replay suite establishes through the gated
        spikes.  `attn.attn_sn`, the dead attention score (:709-711), is `attention_score` on the gated spikes e."""
        Cc, nH, R = q.shape[-1], blk.nH, self._rec_samples
        rows = B_ * N1
        n = rows * nH // R                              # per sample (replicas: its rows are the r-th of R pieces of every step)
        n4 = (n + 3) // 4 * 4                           # (the neuron kernel moves 4 neurons per lane; the padding is not counted)
        # padded PER SAMPLE: the record (T', R, n) of the (T', R, n4) buffer keeps the count kernel's addressing form - R pieces per
        # step, one row of n bytes each, n4 apart
        a = torch.zeros((Tq, R, n4), dtype=torch.float32, device=q.device)
        a[:, :, :n] = q.reshape(Tq, rows, nH, Cc // nH).sum(-1, dtype=torch.float32).view(Tq, R, n)
        g = torch.empty((Tq, R, n4), dtype=torch.uint8, device=q.device)
        self._neuron_fwd(a, g, Tq, 1, R * n4, 0, R * n4, 0, R * n4, blk.sn2_q)
        self._rec_monitor(blk.name + "attn.sn2_q.spiking_neuron.", g[:, :, :n], "flat")
        s = attention_score(e, blk.attn_sn, nH, Tq, B_, N1, self._neuron_fwd, rep=R)
        self._rec_monitor(blk.name + "attn.attn_sn.spiking_neuron.", s, "flat")

    def _rec_monitor(self, name, spikes, layout):
        """A record that goes to the monitor alone (the parity tape does not hold it): u8 spikes, or fp32 ones that are counted as u8."""
        self._to_monitor(name, spikes if spikes.dtype == torch.uint8 else spikes.to(torch.uint8), layout)

    def _neuron_bd(self, x, p, bn=None, out_dtype=torch.uint8, out=None):
        """Neuron over D of a channel-last (B,D,h,w,C) activation, BN fused when given."""
        self._check_cl(x)
        B, D, h, w, Cc = x.shape
        if out is None:
            out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
        a, b = bn if bn is not None else (None, None)
        n = h * w * Cc
        self._neuron_fwd(x, out, D, B, n, D * n, n, D * n, n, p, alpha=a, beta=b, Cch=Cc, inner=1)
        return out

    def _conv3x3(self, s, Wp, Cout, stride=1, bn=None, resid=None, sn=None, membrane=False):
        """3x3 / pad 1 spike convolution on (B,D,h,w,Cin) u8 -> (B,D,oh,ow,Cout): fp32 (BN, + resid) or, with `sn`,
        spikes of the fused BN + neuron over D; with `membrane` as well, (fp32 BN + resid, spikes of SN(that)) from one launch.
        The route (conv3x3_route) says which `_conv_<form>` helper launches it and how many samples each launch takes; every launch
        writes its slice of the outputs."""
        B, D, h, w, Cin = s.shape
        route = conv3x3_route(B, D, h, w, Cin, Cout, stride, getattr(Wp, "digits", None) is not None, None if sn is None else sn.kind, self.replicas)
        shape = (B, D, (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1, Cout)
        m = torch.empty(shape, dtype=torch.float32, device=s.device) if sn is None or membrane else None
        sp = torch.empty(shape, dtype=torch.uint8, device=s.device) if sn is not None else None
        n = route.samples
        if m is None:
            resid = None                                          # (the shortcut goes into the membrane; spikes alone take none)
        elif resid is not None and n < B:
            resid = resid.view(shape)                             # (callers also hand it over as (B * D, oh, ow, Cout) images)
        launch, io = getattr(self, "_conv_" + route.form), (s, resid, m, sp)
        for b0 in range(0, B, n):
            launch(Wp, stride, bn, sn, *(io if n == B else [None if t is None else t[b0:b0 + n] for t in io]))
        return m if sn is None else ((m, sp) if membrane else sp)

    @staticmethod
    def _spike_conv(W, stride, bn, sn, s, resid, m, sp):
        """ONE 3x3 launch on the weights W (16-bit planes or digits): fp32 epilogue into m; with `sn`, spikes into sp (and the membrane
        into m where the caller wants it)."""
        B, D, h, w, Cin = s.shape
        oh, ow = (sp if m is None else m).shape[2:4]
        a, b = bn if bn is not None else (None, None)
        hip.spike_conv2d(s, W, B * D, h, w, Cin, oh, ow, 3, 3, stride, (-1, 0, 1), (-1, 0, 1), out=m, out_spike=sp, alpha=a, beta=b, resid=resid,
                         sn=sn, sn_T=D if sn is not None else 0, pos=(B * oh * ow, oh * ow, D * oh * ow, oh * ow))

    def _conv_then_neuron(self, W, stride, bn, sn, s, resid, m, sp):
        """Convolution with BN into the membrane (a scratch one when the caller wants spikes only), then the bare neuron."""
        if m is None:
            m = torch.empty(sp.shape, dtype=torch.float32, device=s.device)
        self._spike_conv(W, stride, bn, None, s, resid, m, None)
        self._neuron_bd(m, sn, out=sp)

    def _conv_stream(self, Wp, *launch):
        self._spike_conv(Wp, *launch)

    def _conv_wres(self, Wp, *launch):
        self._spike_conv(Wp.digits, *launch)

    def _conv_wres_neuron(self, Wp, *launch):
        self._conv_then_neuron(Wp.digits, *launch)

    def _conv_smallm(self, Wp, stride, bn, sn, *io):
        try:
            self._spike_conv(Wp.digits, stride, bn, sn, *io)
        except hip.SdfError as e:
            # the Python mirror `smallm_conv_applicable` admits a shape the library's own rule refuses (size / alignment, 31-bit sizes,
            # an unusual tau: ADVICE r4 / r5): the 16-bit planes are still here - the streaming kernels serve it
            if e.rc not in (hip.E_SHAPE, hip.E_ALIGN):
                raise
            if sn is not None and sn.kind == "psn":
                # a PSN res-block was sent here because the small-M kernel fuses its neuron; refused, it runs as the fp32
                # convolution + the neuron kernel, not on the streaming kernels' fused epilogue
                self._conv_then_neuron(Wp, stride, bn, sn, *io)
            else:
                self._conv_stream(Wp, stride, bn, sn, *io)

    def _resblock(self, m, rb, s1=None, next_sn=None):
        """MS_ResBlock on a (B,D,h,w,C) membrane: SN -> conv+BN+SN (one kernel) -> conv+BN+identity (one kernel)
        (reference Spiking_modules.py:906-933).  `s1` = SN1(m) if the producer of m already made it; with `next_sn` the
        second convolution also emits the spikes of the NEXT layer's neuron on its output: returns (m', SN_next(m'))."""
        B, D, h, w, _ = m.shape
        if s1 is None:
            s1 = self._neuron_bd(m, rb.sn1)
        self._rec(rb.name + "sn1.spiking_neuron.", s1, "BDHWC->TBCHW")
        fus = conv3x3_carries_neuron(B, D, h, w, rb.C, rb.C, 1, getattr(rb.w1, "digits", None) is not None, rb.sn2.kind, self.replicas)
        if fus:
            s2 = self._conv3x3(s1, rb.w1, rb.C, bn=rb.bn1, sn=rb.sn2)
        else:       # few rows: the fp32 epilogue can split K over the chip; neuron as its own launch
            s2 = self._neuron_bd(self._conv3x3(s1, rb.w1, rb.C), rb.sn2, bn=rb.bn1)
        self._rec(rb.name + "sn2.spiking_neuron.", s2, "BDHWC->TBCHW")
        if next_sn is not None and fus:
            return self._conv3x3(s2, rb.w2, rb.C, bn=rb.bn2, resid=m, sn=next_sn, membrane=True)
        m2 = self._conv3x3(s2, rb.w2, rb.C, bn=rb.bn2, resid=m)
        return (m2, self._neuron_bd(m2, next_sn)) if next_sn is not None else m2

    # ------------------------------------------------------------------ stages (each usable stand-alone in tests)
    def patch_embed(self, x):
        """(B,bins,2,H,W) -> membrane (B,D,H/4,W/4,C), channel-last (reference Spiking_modules.py:1770-1790)."""
        xv = x                                                   # the voxel as handed over (the kernel reads its first num_bins bins in place)
        if x.size(1) > self.num_bins:
            x = x[:, :self.num_bins]
        B, T = x.shape[0], self.num_steps
        H, W = x.shape[-2:]
        num_ch = self.num_bins * 2 // T
        # head: real-valued 2-channel input -> conv + BN + SN as one kernel that reads the voxel in place (channel ci of step t is
        # polarity ci % 2 of bin (ci // 2) * T + t; shapes outside its build: re-layout + library convolution, then BN + SN
        # fused in the neuron kernel)
        if self._head_fused(T, H, W, num_ch) and xv.is_contiguous():
            s = hip.head_conv_sn(xv, self.head_w_oihw, B, T, H, W, self.head_sn, alpha=self.head_bn[0], beta=self.head_bn[1],
                                 voxel_bins=xv.shape[1])
        else:
            ev = x.permute(0, 2, 3, 4, 1)                                                 # (B,2,H,W,bins)
            xr = torch.stack([ev[:, i % 2, :, :, (i // 2) * T:(i // 2 + 1) * T] for i in range(num_ch)], -1)   # (B,H,W,T,ch)
            xr = xr.permute(0, 3, 1, 2, 4).contiguous().view(B * T, H, W, num_ch)           # NHWC, image = (b,t)
            y = F.conv2d(xr.permute(0, 3, 1, 2), self.head_w, None, 1, 1).contiguous(memory_format=torch.channels_last)
            s = self._neuron_bd(y.permute(0, 2, 3, 1).view(B, T, H, W, -1), self.head_sn, bn=self.head_bn)
        self._rec(self.pe_name + "head.sn.spiking_neuron.", s, "BDHWC->TBCHW")
        # every membrane of the patch embedding leaves its convolution together with the spikes of the neuron that reads it
        sns = [rb.sn1 for rb in self.pe_res] + [self.proj_sn]
        C0 = self.conv_w.shape[1]
        fus = conv3x3_carries_neuron(B, T, H, W, s.shape[-1], C0, 2, getattr(self.conv_w, "digits", None) is not None, sns[0].kind, self.replicas)
        if fus:
            m, s1 = self._conv3x3(s, self.conv_w, C0, stride=2, bn=self.conv_bn, sn=sns[0], membrane=True)
        else:
            m = self._conv3x3(s, self.conv_w, C0, stride=2, bn=self.conv_bn)
            s1 = self._neuron_bd(m, sns[0])
        for i, rb in enumerate(self.pe_res):
            m, s1 = self._resblock(m, rb, s1=s1, next_sn=sns[i + 1])
        # PED projection: 1x1 stride-2 shortcut on the (real-valued) membrane + SN -> conv3x3 s2 -> BN, summed in the epilogue
        Bm, Dm, h, w, Cc = m.shape
        self._rec(self.pe_name + "proj.sn.spiking_neuron.", s1, "BDHWC->TBCHW")
        if hip.pointwise_conv_supported(Cc, self.proj_res_w2.shape[0]):                # exact fp32 MFMA (csrc/pointwise_conv.hip)
            res = hip.pointwise_conv_f32(m.view(B * T, h, w, Cc), self.proj_res_w2, 2, self.proj_res_b)
        else:
            res = F.conv2d(m.view(B * T, h, w, Cc).permute(0, 3, 1, 2), self.proj_res_w, self.proj_res_b, 2)
            res = res.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        return self._conv3x3(s1, self.proj_w, self.proj_w.shape[1], stride=2, bn=self.proj_bn, resid=res)

    def _head_fused(self, T, H, W, num_ch):
        """Whether the head convolution runs with BN and its neuron as one kernel (else: library convolution, then BN + neuron)."""
        return hip.head_conv_sn_supported(T, H, W, num_ch, self.head_w_oihw.shape[0])

    def _zsrc_map(self, rowmap, B_, Tq, N1, nH, x_rows, key):
        key = ("zsrc", nH, self.replicas) + key
        if key not in self._maps:
            B = key[3]
            if self.replicas and B > 1:
                _, D, H, W, ws, ss = key[3:]
                m1, nW = self._slice_map_1(D, H, W, ws, ss)
                z1 = hip.window_zsrc_map(m1, nW, Tq, N1, nH, x_rows // B)
                self._maps[key] = hip.replica_zsrc_map(z1, nW, B, Tq, N1, nH * 32)
            else:
                self._maps[key] = hip.window_zsrc_map(rowmap, B_, Tq, N1, nH, x_rows)     # built on the device, cached per shape
        return self._maps[key]

    def attention(self, x, blk: _Block, score_out=None, emit=None):
        """x (B,D,H,W,C) += SSA(x), in place (reference Spiking_swin_transformer3D.py:781-821, 661-717, :840).  `score_out` (a list)
        also receives the block's attention score (T', B_, Wh, Ww, C) - `return_attention=True` (:807-808) without abandoning x.
        `emit` = (u8 buffer, neuron): on the wide stages the projection's launch also leaves SN(x) over D there (the MLP's first
        neuron, csrc/ms_wide.hip); `self._emitted` says whether it did."""
        self._check_cl(x)
        B, D, H, W, Cc = x.shape
        ws, ss = get_window_size((D, H, W), blk.window_size, blk.shift_size)
        if tuple(ws) != tuple(blk.window_size):
            # the reference clamps the window (:786) and then cannot view its positional encoding, sized for the nominal window, as
            # (T', 1, Wh, Ww, C) (:678, RuntimeError); refused here as well instead of reading the table with the wrong pitch
            raise hip.SdfError(f"feature map {(D, H, W)} is smaller than the window {tuple(blk.window_size)}: the positional encoding of "
                               "Spiking_QK_WindowAttention3D is defined for the nominal window only (reference Spiking_swin_transformer3D.py:678)")
        rowmap, B_ = self._slice_map(B, D, H, W, ws, ss)
        Tq, N1 = ws[0], ws[1] * ws[2]
        rep_windows = B_ // B if self.replicas and B > 1 else 0
        if rep_windows and (self.tape is not None or score_out is not None):     # (a monitor counts per sample: _rec)
            raise hip.SdfError("the parity tape and log=True follow one forward: run them without replicas")
        # one C-ABI call: neuron over the gathered slices -> q|k spike GEMM (+BN, +PE, neurons fused) -> token gate ->
        # projection spike GEMM through the head scramble with bias + BN + scatter + residual (csrc/qk_attn.hip)
        keep = [] if score_out is not None else None
        if self.taped:
            # the slice spikes are overwritten by the gate inside the call: the tape runs the same kernel on the same input first
            rows, keep = B_ * N1, []
            xs = torch.empty((Tq, rows, Cc), dtype=torch.uint8, device=x.device)
            self._neuron_fwd(x, xs, Tq, 1, rows * Cc, 0, 0, 0, rows * Cc, blk.sn_proj, rowmap=rowmap, rowlen=Cc)
            self._rec(blk.name + "attn.proj_sn.spiking_neuron.", xs, "flat")
        info = {}
        zsrc = self._zsrc_map(rowmap, B_, Tq, N1, blk.nH, B * D * H * W, (B, D, H, W, tuple(ws), tuple(ss))) if Cc >= _WIDE_MINC and Tq == 2 else None
        kw = dict(qk=blk.qk) if blk.qk is not None else dict(q_lin=blk.q, k_lin=blk.k, pe=blk.pe)
        hip.qk_attn(x, rowmap, B_, Tq, N1, blk.nH, blk.p, blk.sn_proj, blk.sn_q, blk.sn_k, blk.sn2_q, keep_ws=keep, x_src=zsrc, emit=emit,
                    info=info, rep_windows=rep_windows, **kw)
        if score_out is not None:
            # the gate's output replaced the slice spikes at the head of the workspace (csrc/qk_attn.hip)
            e = keep[0][:Tq * B_ * N1 * Cc].view(Tq, B_ * N1, Cc)
            score_out.append(attention_score(e, blk.attn_sn, blk.nH, Tq, B_, N1).view(Tq, B_, ws[1], ws[2], Cc))
        if keep and self.taped:
            M = Tq * B_ * N1
            qk = keep[0][(M * Cc + 255) // 256 * 256:][:M * 2 * Cc]
            q, k = (qk.view(M, 2 * Cc)[:, :Cc], qk.view(M, 2 * Cc)[:, Cc:]) if blk.qk is not None else (qk[:M * Cc], qk[M * Cc:])
            self._rec(blk.name + "attn.sn_q.spiking_neuron.", q.reshape(Tq, B_ * N1, Cc), "flat")
            self._rec(blk.name + "attn.sn_k.spiking_neuron.", k.reshape(Tq, B_ * N1, Cc), "flat")
            if self.monitor is not None:
                self._rec_gates(blk, q.reshape(Tq, B_ * N1, Cc), keep[0][:M * Cc].view(Tq, B_ * N1, Cc), Tq, B_, N1)
        self._emitted = bool(info.get("emitted"))
        return x

    def mlp(self, x, blk: _Block, ws=None, s1_ready=False, emit_next=None):
        """x (B,D,H,W,C) += MLP(x) over the true time axis D, in place (reference :164-181, :845).  `ws` / `s1_ready`: the caller's
        workspace with SN1's spikes already at its head (wide stages: left there by the attention's projection); `emit_next`: see
        _next_spikes."""
        self._check_cl(x)
        keep = [] if self.taped else None
        hip.ms_mlp(x, blk.fc1, blk.fc2, blk.sn1, blk.sn2, keep_ws=keep, ws=ws, s1_ready=s1_ready, emit_next=emit_next)      # one C-ABI call (csrc/qk_attn.hip: sdf_ms_mlp_fwd)
        if keep:
            B, D, H, W, Cc = x.shape
            tok = B * D * H * W
            self._rec(blk.name + "mlp.sn1.spiking_neuron.", keep[0][:tok * Cc].view(B, D, H, W, Cc), "BDHWC->TBHWC")
            self._rec(blk.name + "mlp.sn2.spiking_neuron.", keep[0][(tok * Cc + 255) // 256 * 256:][:tok * blk.fc1.N].view(B, D, H, W, -1), "BDHWC->TBHWC")
        return x

    def swin_block(self, x, s, i, emit_next=None):
        blk = self.stages[s][i]
        last = self.scores is not None and i == len(self.stages[s]) - 1          # log=True: the last block of every stage (:1090-1105)
        # wide stages: the projection emits the MLP's first spikes (tiled hand-over layout; the tape / score paths keep row-major spikes
        # and let the MLP run its own first neuron)
        ws = hip.ms_mlp_workspace(x, blk.fc1.N) if x.shape[-1] >= _WIDE_MINC and not self.taped and not last else None
        self.attention(x, blk, self.scores if last else None, emit=(ws, blk.sn1) if ws is not None else None)
        return self.mlp(x, blk, ws=ws, s1_ready=self._emitted, emit_next=emit_next)

    def _tail_kwargs(self):
        """encoder() arguments of forward(): the neuron that reads the last stage's output first (MS_ResBlock.sn1 of the bottleneck)."""
        return {"tail_sn": self.unet_res[0].sn1} if self.unet_res else {}

    def _next_spikes(self, x, blk, sn):
        """(u8 buffer, neuron) for the MLP of `blk` to fill with SN(x after its update) - the first neuron of the layer behind the
        stage - or None where that MLP does not run on the wide-stage kernels (the layer then runs its own neuron)."""
        if x.shape[-1] < _WIDE_MINC or not hip.ms_mlp_is_wide(x, blk.fc1, blk.fc2, blk.sn1, blk.sn2, emit_sn=sn):
            return None
        return torch.empty(x.shape, dtype=torch.uint8, device=x.device), sn

    def patch_merge(self, x, s, packed=None, spikes=None):
        """(B,D,H,W,C) -> (B,D,H/2,W/2,2C) (reference :952-974).  `spikes` = SN(x) (B,D,H,W,C) u8 when the stage's last MLP emitted
        them: the 2x2 concatenation is then index arithmetic inside the reduction GEMM (hip.ms_patch_merge)."""
        lin, sn = self.merges[s] if packed is None else packed
        self._check_cl(x)
        B, D, H, W, Cc = x.shape
        name = f"sttmultires_unet.encoders.swin3d.layers.{s}.downsample.sn.spiking_neuron."
        if spikes is None and getattr(lin, "digits", None) is not None and D in (10, 20) and sn.kind in hip.KIND:
            # the stage's last MLP did not emit them (stage 0: it runs on the one-launch fp16-plane kernel): the neuron as a plain
            # launch over x, then the same digit-plane reduction with the 2x2 concatenation as operand addressing - 8 + 19 us at the
            # first merge of the shipped model against 33 us for the gathered neuron + spike GEMM below
            spikes = self._neuron_bd(x, sn)
        if spikes is not None:
            out = hip.ms_patch_merge(spikes, lin)
            if out is not None:
                if self.tape is not None:        # the tape holds the reference's (T, B, H/2, W/2, 4C) concatenation
                    src, H2, W2 = merge_row_map(B, D, H, W)
                    idx = torch.from_numpy(src.reshape(-1).astype("int64")).to(x.device)
                    flat = torch.cat([spikes.view(-1, Cc), spikes.new_zeros(1, Cc)], 0)
                    self.tape.append((name, flat[idx].view(D, B, H2, W2, 4 * Cc), "flat"))
                if self.monitor is not None:
                    # the concatenation moves every row of a (sample, step) once and adds zero rows where a size is odd: the spikes of
                    # a sample and step are those of `spikes`, counted where they lie (nothing gathered, nothing allocated); the
                    # denominator is the concatenation's (elements per step of the whole record)
                    self.monitor.record(name, spikes, "BDHWC->TBHWC", elements=B * out.shape[2] * out.shape[3] * 4 * Cc,
                                        **({"samples": self._rec_samples} if self._rec_samples > 1 else {}))
                return out
        return self._patch_merge_gathered(x, lin, sn, name)

    def _patch_merge_gathered(self, x, lin, sn, name):
        """The merge as the reference lays it out: the neuron over the gathered 2x2 concatenation (a zero row where the size is odd),
        then the reduction product with BN."""
        B, D, H, W, Cc = x.shape
        rowmap, H2, W2, out_map = self._merge_map(B, D, H, W)
        rows = B * H2 * W2
        sp = torch.empty((D * rows, 4 * Cc), dtype=torch.uint8, device=x.device)
        self._neuron_fwd(x, sp, D, 1, rows * 4 * Cc, 0, 0, 0, rows * 4 * Cc, sn, rowmap=rowmap, rowlen=Cc)
        self._rec(name, sp.view(D, B, H2, W2, 4 * Cc), "flat")
        out = torch.empty((B, D, H2, W2, lin.N), dtype=torch.float32, device=x.device)
        hip.spike_gemm(sp, lin.Wp, out, D * rows, lin.N, 4 * Cc, alpha=lin.alpha, beta=lin.beta, out_rowmap=out_map)
        return out

    def encoder(self, x, tail_sn=None):
        """-> per-stage features, channel-last (B,D,h,w,C) (reference :1223-1246 + Spiking_STSwinNet.py:77-85).  `tail_sn` = the first
        neuron of whatever reads the last stage's output: where the last MLP can emit its spikes they are left in `self.tail_spikes`."""
        y = self.patch_embed(x)
        feats = []
        self.tail_spikes = None
        for s, blocks in enumerate(self.stages):
            nxt_sn = self.merges[s][1] if s < len(self.merges) else tail_sn
            emit = None
            for i in range(len(blocks)):
                if i == len(blocks) - 1 and nxt_sn is not None:
                    emit = self._next_spikes(y, blocks[i], nxt_sn)
                y = self.swin_block(y, s, i, **({"emit_next": emit} if emit is not None else {}))
            feats.append(y)                                 # the merge writes a new tensor; nothing touches y after this
            if s < len(self.merges):
                y = self.patch_merge(y, s, **({"spikes": emit[0]} if emit is not None else {}))
            elif emit is not None:
                self.tail_spikes = emit[0]
        return feats

    def _cached(self, key, make):
        if key not in self._deconv:
            self._deconv[key] = make()
        return self._deconv[key]

    def _decoder_weight(self, i, wkey, C1, C2):
        """ConvTranspose2d weight (Cin, Cout, 3, 3) of decoder i in the reference's input-channel order [pred | y | skip] ("ref")
        or in the physical order of the concatenation-free path [y | skip | pred, 0, 0] ("perm")."""
        wdec = self.decoders[i].w
        if wkey == "ref" or i == 0:
            return wdec

        def perm():
            n = wdec.shape[0] - C1 - C2                                   # prediction channels in front (2)
            pad = torch.zeros((4 - n,) + tuple(wdec.shape[1:]), dtype=wdec.dtype, device=wdec.device)
            return torch.cat([wdec[n:n + C1], wdec[n + C1:], wdec[:n], pad], 0).contiguous()
        return self._cached(("wperm", i), perm)

    def _decoder_levels(self, feats, y0):
        """Every decoder level (_Level) decided before anything is launched."""
        levels, (hy, wy, C1), E = [], y0.shape[2:], len(feats)
        for i in range(E):
            B, D, h, w, C2 = feats[E - 1 - i].shape
            same = (hy, wy) == (h, w)
            cin = C1 + C2 + (0 if i == 0 else (4 if same else self.preds[i - 1].nout))
            cout = self.decoders[i].w.shape[1]
            levels.append(_Level(same, cin, deconv_route(B, D, h, w, cin, cout, self.nsplit, self.replicas)))
            hy, wy, C1 = 2 * h, 2 * w, cout
        return levels

    def _prepare_decoder_images(self, feats, y0, out_size, levels):
        """NHWC u8 spike images of every decoder level with the skip slices written by one multi-descriptor neuron launch, or None
        when the pyramid is not regular / a level's head has no one-launch kernel (the per-level path handles those)."""
        E = len(feats)
        if out_size is None or E < 2 or E > 6 or not all(lv.same for lv in levels):
            return None
        imgs, calls, c1 = [], [], y0.shape[-1]
        for i, lv in enumerate(levels):
            skip = feats[E - 1 - i]
            B, D, h, w, C2 = skip.shape
            dec, pr = self.decoders[i], self.preds[i]
            cout = dec.w.shape[1]
            if not (pr.nout == 2 and out_size[0] % (2 * h) == 0 and out_size[1] % (2 * w) == 0 and
                    hip.pred_head_supported(D, cout, out_size[0], out_size[1], 2 * h, 2 * w, pr.sn, self.decoders[i + 1].sn if i + 1 < E else None)):
                return None
            cin, cp, hw = lv.cin, lv.route.cp, h * w
            img = torch.empty((B, D, h, w, cp), dtype=torch.uint8, device=y0.device)
            if i == 0 and cp != cin:
                img[..., cin:].zero_()                                  # (levels >= 1: zeroed by the head of the level above)
            # (the batch elements are the descriptor's outermost dimension: one multi-descriptor launch for the whole batch)
            calls.append(((skip, img.view(-1)[c1:], D, hw, C2, C2, hw * C2, cp, hw * cp, dec.sn), {"rep": (B, D * hw * C2, D * hw * cp)}))
            imgs.append(img)
            c1 = cout
        # level 0's own input y rides in the same launch (its neuron is the level's `sn` too; six descriptors at most)
        self._ready_has_y = len(calls) < 6
        if self._ready_has_y:
            B, D, h0, w0, cy = y0.shape
            hw0, cp0 = h0 * w0, imgs[0].shape[-1]
            calls.append(((y0, imgs[0].view(-1), D, hw0, cy, cy, hw0 * cy, cp0, hw0 * cp0, self.decoders[0].sn), {"rep": (B, D * hw0 * cy, D * hw0 * cp0)}))
        hip.neuron_multi_fwd(calls)
        return imgs

    def _decoder_image(self, i, level, y, skip, preds, ready, carried):
        """-> (NHWC u8 spike image (B,D,h,w,cp) of decoder level i, order of its channels: "perm" / "ref" as _decoder_weight has them):
        SN(skip_concat(pred, skip_concat(y, skip))) on channels (:168-172); the prediction has y's size (both come from z)."""
        same, cin, cp = level.same, level.cin, level.route.cp
        B, D, h, w, C2 = skip.shape
        sn, C1, name = self.decoders[i].sn, y.shape[-1], f"sttmultires_unet.decoders.{i}.sn.spiking_neuron."
        if not same:
            parts = [_center_pad(p, h, w) for p in ([preds[-1][..., :self.preds[i - 1].nout]] if i > 0 else []) + [y, skip]]
            if cp != cin:
                cat = torch.zeros((B, D, h, w, cp), dtype=torch.float32, device=y.device)
                torch.cat(parts, dim=-1, out=cat[..., :cin])
            else:
                cat = torch.cat(parts, dim=-1)
            s = self._neuron_bd(cat, sn)                                  # MS decoder: SN -> ConvT -> BN
            self._rec(name, s[..., :cin], "BDHWC->TBCHW")
            return s, "ref"
        # no concatenation: the decoder's neuron runs on each source and writes its spikes straight into that source's channel slice
        # of the spike image (the transposed-convolution weight rows are permuted to match once, at pack time)
        if ready is not None:
            s, c0 = ready[i], 0                                           # skip slice (and padding) already in place; level 0 takes y now
            srcs = [(y, C1, C1)] if i == 0 and not self._ready_has_y else []
        elif carried is not None:
            s, srcs, c0 = carried, [(skip, C2, C2)], C1                  # [y | . | prediction | zeros] came from the level above
        else:
            s = (torch.zeros if cp != cin else torch.empty)((B, D, h, w, cp), dtype=torch.uint8, device=y.device)
            srcs, c0 = [(y, C1, C1), (skip, C2, C2)] + ([(preds[-1], 4, preds[-1].shape[-1])] if i > 0 else []), 0
        for src, take, pitch in srcs:                                     # (tensor, channels taken, pitch)
            self._slice_neuron(src, take, pitch, s, c0, sn)
            c0 += take
        if self.taped:                                         # the reference's channel order is [prediction | y | skip]
            npred = self.preds[i - 1].nout if i > 0 else 0
            self._rec(name, torch.cat([s[..., C1 + C2:C1 + C2 + npred], s[..., :C1 + C2]], -1), "BDHWC->TBCHW")
        return s, "perm"

    def _slice_neuron(self, src, take, pitch, s, c0, sn):
        """Spikes of `sn` over D on the first `take` channels of src (B,D,h,w,pitch) fp32, into channels c0.. of the image s (B,D,h,w,cp) u8."""
        B, D, h, w, cp = s.shape
        hw = h * w
        for b in range(B):
            self._neuron_fwd(src[b], s[b].view(-1)[c0:], D, hw, take, pitch, hw * pitch, cp, hw * cp, sn)

    def _transposed_conv(self, i, route, s, wkey, wuse):
        """z (B,D,2h,2w,cout) fp32 = BN(ConvTranspose2d(k 3, s 2, p 1, op 1)(s)) of decoder level i, launched as deconv_route decided."""
        form, cp, per = route
        B, D, h, w, _ = s.shape
        bn, cout, imgs = self.decoders[i].bn, wuse.shape[1], B * D
        z = torch.empty((B, D, 2 * h, 2 * w, cout), dtype=torch.float32, device=s.device)
        sv, zv, zrows = s.view(imgs, h, w, cp), z.view(imgs, 2 * h, 2 * w, cout), z.view(imgs, 4 * h * w, cout)
        if form.startswith("taps"):
            planes = self._cached(("taps", i, cp, wkey), lambda: deconv_tap_weights(wuse, cp, self.nsplit))
            taps = planes if form == "taps_stream" else (planes.digits if form == "taps_smallm" else planes.digits_rm)
            Y = torch.empty((imgs * h * w, 9 * cout), dtype=torch.float32, device=s.device)
            mc = per * h * w
            for m0 in range(0, imgs * h * w, mc):
                hip.spike_gemm(s.view(-1, cp)[m0:m0 + mc], taps, Y[m0:m0 + mc], mc, 9 * cout, cp)
            hip.deconv_col2im(Y, imgs, h, w, cout, alpha=bn[0], beta=bn[1], out=z)
        elif form == "one_product":
            pl, a4, b4 = self._cached(("d2x2", i, cp, wkey), lambda: (hip.pack_deconv2x2_weight(wuse, cp), bn[0].repeat(4).contiguous(),
                                                                      bn[1].repeat(4).contiguous()))
            for i0 in range(0, imgs, per):
                hip.spike_deconv3x3s2(sv[i0:i0 + per], pl, per, D, h, w, cp, cout, alpha=a4, beta=b4, out=zv[i0:i0 + per], tiled_bn=True)
        elif form == "classes_multi":
            # (replicas: the classes, and their row maps, of the first D images serve every sample's slice)
            classes = self._cached((i, per // D, D, h, w, wkey), lambda: deconv_classes(wuse, per, h, w, cp, self.nsplit, self.device))
            for i0 in range(0, imgs, per):
                hip.spike_conv2d_multi(sv[i0:i0 + per], classes, per, h, w, cp, h, w, zrows[i0:i0 + per], alpha=bn[0], beta=bn[1])
        else:
            # (the row map of the first n images serves every chunk)
            for cls in self._cached((i, B, D, h, w, wkey), lambda: deconv_classes(wuse, imgs, h, w, cp, self.nsplit, self.device)):
                for i0 in range(0, imgs, per):
                    n = min(per, imgs - i0)
                    hip.spike_conv2d(sv[i0:i0 + n], cls["Wp"], n, h, w, cp, h, w, cls["KH"], cls["KW"], 1, cls["dy"], cls["dx"],
                                     out=zrows[i0:i0 + n], alpha=bn[0], beta=bn[1], out_rowmap=cls["rowmap"][:n * h * w])
        return z

    def _prediction(self, i, z, feats, out_size, levels, ready):
        """Prediction head of level i on z (B,D,H2,W2,cout) -> (prediction (B,D,H2,W2,>= nout) fp32 or None, the next level's spike image
        with its [y | prediction] slices written, or None).  MS pred: SN -> conv1x1 (+bias), 2 outputs."""
        B, D, H2, W2, cout = z.shape
        pr, E, name = self.preds[i], len(feats), f"sttmultires_unet.preds.{i}.sn.spiking_neuron."
        nxt_skip = feats[E - 2 - i] if i + 1 < E else None
        fs = out_size if out_size is not None and out_size[0] % H2 == 0 and out_size[1] % W2 == 0 else None
        if not (pr.nout == 2 and self._pred_head_fused(D, cout, fs[0] if fs else H2, fs[1] if fs else W2, H2, W2, pr.sn,
                                                       self.decoders[i + 1].sn if nxt_skip is not None else None)
                and B * D * H2 * W2 * max(cout, 16) * 4 < 1 << 40):
            sp = self._neuron_bd(z, pr.sn)
            self._rec(name, sp, "BDHWC->TBCHW")
            po = torch.empty((B * D * H2 * W2, 32), dtype=torch.float32, device=z.device)
            hip.spike_gemm(sp, pr.planes, po, po.shape[0], 32, cout, bias=pr.bias)
            return po.view(B, D, H2, W2, 32), None                        # columns nout.. are exactly zero (zero weight rows, zero bias)
        # its time sum + upsampling, and the next level's [y | prediction] spikes - one launch, z read once (csrc/pred_head.hip)
        nxt = carried = None
        if nxt_skip is not None and levels[i + 1].same:
            cin_n, cp_n = levels[i + 1].cin, levels[i + 1].route.cp
            carried = ready[i + 1] if ready is not None else torch.empty((B, D, H2, W2, cp_n), dtype=torch.uint8, device=z.device)
            nxt = (carried, self.decoders[i + 1].sn, 0, cin_n - 4, (cin_n, cp_n - cin_n))
        pred, self._flows[i], sp = hip.pred_head(z, pr.w, pr.b, pr.sn, fs[0] if fs else None, fs[1] if fs else None,
                                                 want_pred=self.taped or fs is None or (i + 1 < E and nxt is None),
                                                 nxt=nxt, keep=self.taped)
        if sp is not None:
            self._rec(name, sp, "BDHWC->TBCHW")
        return pred, carried

    # whether a level's prediction head runs as one launch with its neuron inside (the unfused plan answers no)
    @staticmethod
    def _pred_head_fused(*a):
        return hip.pred_head_supported(*a)

    def unet_tail(self, feats, out_size=None, s1=None):
        """res-blocks + decoders + per-scale predictions on channel-last (B,D,h,w,C) features
        (reference Spiking_STSwinNet.py:161-182).  `s1` = the first res-block's SN1(feats[-1]) where the encoder's last MLP emitted it
        (encoder(..., tail_sn=)).  Returns the per-scale predictions (B,D,h',w',2) fp32; with `out_size` = (H, W)
        the flow maps (time sum + nearest upsampling, reference :289-303) of the levels whose prediction head ran as one launch
        are left in `self._flows` (None where the three-launch form ran: forward() calls sdf_flow_out_fwd for those)."""
        y = feats[-1]
        for i, rb in enumerate(self.unet_res):                # a block's second convolution also emits the next block's first spikes
            nxt = self.unet_res[i + 1].sn1 if i + 1 < len(self.unet_res) else None
            r = self._resblock(y, rb, s1=s1, next_sn=nxt)
            y, s1 = r if nxt is not None else (r, None)
        preds, E = [], len(feats)
        self._flows = [None] * E
        levels = self._decoder_levels(feats, y)
        # Regular pyramid (every level twice the size of the one before, every prediction head on its one-launch kernel): the
        # spike images of ALL levels are laid out now and the decoders' neuron on the four skip tensors - four small launches
        # before - is ONE launch (sdf_neuron_multi_fwd); the [y | prediction] slices arrive from the level above's head.
        ready = self._prepare_decoder_images(feats, y, out_size, levels) if not self.taped else None
        carried = None          # this level's spike image with the [y | prediction] slices already written by the previous level's head
        for i, level in enumerate(levels):
            skip = feats[E - 1 - i]
            s, wkey = self._decoder_image(i, level, y, skip, preds, ready, carried)
            y = self._transposed_conv(i, level.route, s, wkey, self._decoder_weight(i, wkey, y.shape[-1], skip.shape[-1]))
            pred, carried = self._prediction(i, y, feats, out_size, levels, ready)
            preds.append(pred)
        return [None if p is None else p[..., :self.preds[0].nout] for p in preds]

    def forward(self, x, scores=None, replicas=False):
        """(B,bins,2,H,W) fp32 on the GPU -> list of E flow maps (B,2,H,W) (reference :278-305).  `scores` (a list) receives the
        `log=True` output (:283-284): the attention score (T', B_, Wh, Ww, C) of the last block of every stage - what the reference's
        `get_layer_attention_scores` is written to return (its own call chain raises: oracle/sdformer_oracle.py `swin_encoder`).
        `replicas`: the B samples are B INDEPENDENT batch-1 forwards served by one launch sequence - flow i is bit-equal to
        forward(x[i:i+1]) - instead of one reference batch (whose samples window_partition_v2's raw view couples): the
        only difference is the window tables (hip.replica_slice_map / replica_zsrc_map), every kernel sees B times the rows."""
        if not x.is_cuda:
            raise hip.SdfError("input must be a GPU tensor (no CPU fallback)")
        x = x.float().contiguous()
        H, W = x.shape[-2:]
        self.scores = scores
        if replicas and self.num_steps not in (10, 20):
            # other step counts leave layers on the streaming kernels (no digit form at T = 5: the MDR config), whose split-K plans follow the
            # row count - the caller (forward_replicas) serves those models one sample at a time
            raise hip.ReplicaGeometryError(f"replicas are built for T = 10 / 20 (digit kernels throughout), not T = {self.num_steps}")
        self.replicas = bool(replicas)
        self._rec_samples = x.shape[0] if replicas else 1
        try:
            feats = self.encoder(x, **self._tail_kwargs())
            self.scores = None
            preds = self.unet_tail(feats, out_size=(H, W), **({"s1": self.tail_spikes} if getattr(self, "tail_spikes", None) is not None else {}))
        finally:
            self.scores = None
            self.replicas = False
            self._rec_samples = 1
        self.tail_spikes = None
        # sum over time + nearest upsampling to the input size: done by the prediction head's launch, else one small kernel per scale
        return [f if f is not None else hip.flow_out(p, H, W, H / p.shape[2], W / p.shape[3]) for p, f in zip(preds, self._flows)]
