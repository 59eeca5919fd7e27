"""Training path of the MS SDformerFlow models (BASELINE config 4): train-mode forward under
autograd, the supervised loss, one optimiser step, and the data-parallel gradient all-reduce.

What is hand-written HIP here: every spiking neuron, forward AND backward (`autograd.LIFFunction` / `PSNFunction` / `PLIFFunction` /
`SLTTFunction` / `GLIFFunction` -> csrc/neuron.hip, csrc/neuron_bwd.hip, csrc/glif.hip; 105 neuron calls per forward), the batch-statistics BatchNorm, the token gate, and -
since round 5 - ALL THREE products of every Linear layer (`autograd.LinearHipFunction`: forward and dX on csrc/linear_train.hip,
dW on csrc/linear_dw.hip: 35 ms of library fp32 GEMM -> 13 ms; no rocBLAS GEMM of a Linear layer is left in a step) and the forward and
weight gradient of the MS_ResBlock convolutions (`autograd.Conv3x3HipFunction`: products over zero-ringed channels-last pixel rows).
The other dense products - the convolutions' dX, the remaining convolutions' forward and dW - are library work through torch on the
same stream (MIOpen); their replacements are the next row.  Behind the backward pass, with a `BucketAdamW`: the per-parameter gradient
statistics (`vis.store_grads`), the clip coefficient and the AdamW update on the flat buckets (csrc/grad_step.hip), without a host
synchronisation - also under fp16 autocast with a `LossScaler` (torch.amp.GradScaler's arithmetic on the device: a step with a
non-finite gradient is skipped by the kernels) and with gradient accumulation (`num_acc`: the running sum is clipped in place);
with any other optimiser torch's clip_grad_norm_ and step.  Between the two, opt-in (`train_step(head="hip")`): the multi-scale loss
and its gradient on the decoder levels' raw predictions in two launches (`flow_loss_hip`, csrc/flow_loss.hip); the default head is
the torch composition `flow_loss_supervised`.  Nothing here touches `oracle/`, and CPU
tensors are refused by the neuron kernels (`SdfError`).

Reference semantics mirrored (file:line under /root/reference):
  model forward           models/STSwinNet_SNN/Spiking_STSwinNet.py:278-305, 161-182
  patch embedding         models/STSwinNet_SNN/Spiking_modules.py:1770-1790 (+ :291-296, :339-347, :811-819, :906-933)
  stage / block / SSA     models/STSwinNet_SNN/Spiking_swin_transformer3D.py:1065-1088, 824-847, 781-821
  QK attention            ...:661-717      window_partition_v2 :100-113    window_reverse swin_transformer3D_v2.py:52-65
  MLP / patch merging     ...:164-181 / :952-974
  BatchNorm in train mode spikingjelly layer.BatchNorm2d, multi-step: flatten (T,B) -> nn.BatchNorm2d (batch statistics)
  DropPath                timm 0.6.13 `drop_path` (per-sample Bernoulli keep mask / keep_prob), SSA branch only (:840)
  loss                    loss/flow_supervised.py:80-105 (gamma None), :14-30
  step                    train_flow_parallel_supervised_SNN.py:233-336 (reset, forward, loss, backward, clip 100, AdamW)
  loader item -> step     ...:155-171, :241-308 (crop, flips, drop, split, min-max, threshold, mask * event_mask): `prepare_train_item`
                          on csrc/prepare_chunk.hip (hip.augment_chunk), `train_step_from_item`
  MDR loader item -> step MDR_dataloader/loader_utils.py:244-341, MDR.py:218-241, train_mdr_supervised_SNN.py:209-276 (rescale, flow *
                          scale, flips, crop, valid, cat, split, min-max, threshold, mask * event_mask): `prepare_mdr_item` on
                          csrc/prepare_chunk.hip (hip.augment_resize_chunk), `train_step_from_mdr_item`
  data parallelism        the reference wraps the model in DataParallel: replicas, local batch statistics, summed
                          gradients; here one process per GPU and ONE bucketed all-reduce(sum)/world per step (RCCL)
"""
import os

import torch
import torch.nn.functional as F

from . import hip
from .STSwinNet_SNN.Spiking_submodules import GatedLIFNode, ParametricLIFNode, SLTTLIFNode


# ---------------------------------------------------------------------------------------------- layers
# Forward of the Linear layers in the training path: 0 = library F.linear (default); 2 / 3 = the inference path's spike GEMM
# with that many weight planes and the activation saved as 1-byte spikes.  Measured at local batch 4: same parity (block-level
# gradients still equal the reference fixture element for element), 2.5 GiB less memory, but the step is SLOWER (fp32 123 ->
# 130 ms: u8 conversion + per-step weight split + fp32 re-expansion in the backward; under bf16 autocast 95 -> 114 ms because
# the backward products leave autocast) - so it stays off until the backward products are spike-aware too (docs/history/DESIGN_rounds1-5.md, round-2 list item 4).
SPIKE_LINEAR_PLANES = 0
# Weight gradient of the Linear layers on csrc/linear_dw.hip (round 5; SDF_TRAIN_LINEAR_DW=0: the library product, for A/B runs)
LINEAR_DW_HIP = os.environ.get("SDF_TRAIN_LINEAR_DW", "1") != "0"
# Forward and dX of the Linear layers on csrc/linear_train.hip (fp32 path; SDF_TRAIN_LINEAR=0: the library products)
LINEAR_HIP = os.environ.get("SDF_TRAIN_LINEAR", "1") != "0"
# ... and of the MS_ResBlock convolutions (3x3 / stride 1 / pad 1 on spikes; SDF_TRAIN_CONV_DW=0: MIOpen's)
CONV_DW_HIP = os.environ.get("SDF_TRAIN_CONV_DW", "1") != "0"
# ... and their forward (SDF_TRAIN_CONV_FWD=0: MIOpen's; the ringed rows are then made in the backward)
CONV_FWD_HIP = os.environ.get("SDF_TRAIN_CONV_FWD", "1") != "0"


def _linear(x, lin, spikes=True):
    """Linear of the training path.  `spikes` (the caller's statement, as `_conv_seq`'s): x holds 0 / 1 values only - every Linear of
    the MS models is fed by a neuron or by the token gate - which is what the hand-written products need: they keep the top 16 bits
    of the activation (csrc/linear_train.hip, linear_dw.hip), exact for spikes and for nothing else.  `spikes=False`: F.linear.
    SDF_DEBUG_CHECKS=1 verifies the statement on the host (one synchronisation per call)."""
    if not spikes:
        return F.linear(x, lin.weight, lin.bias)
    if hip.sw("SDF_DEBUG_CHECKS", "") == "1" and not bool(((x == 0) | (x == 1)).all()):
        raise hip.SdfError("_linear(spikes=True) was handed values other than 0 / 1: the 16-bit-plane products would truncate them")
    K, N = lin.weight.shape[1], lin.weight.shape[0]
    if SPIKE_LINEAR_PLANES and K % 32 == 0 and N % 32 == 0:
        from .autograd import SpikeLinearFunction
        return SpikeLinearFunction.apply(x, lin.weight, lin.bias, SPIKE_LINEAR_PLANES)
    if LINEAR_DW_HIP and x.is_cuda and hip.linear_dw_applicable(x.numel() // K, N, K):
        from .autograd import LinearDwFunction, LinearHipFunction
        if LINEAR_HIP and not torch.is_autocast_enabled():               # (bf16 autocast keeps the library's bf16 forward / dX)
            return LinearHipFunction.apply(x, lin.weight, lin.bias)
        return LinearDwFunction.apply(x, lin.weight, lin.bias)
    return F.linear(x, lin.weight, lin.bias)


def _bn(x_nc, bn):
    """Batch-statistics BatchNorm over dim 1 of (N, C, H, W) with the module's parameters; running stats updated in place."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if hip.bn_train_nchw_supported(x_nc):
        from .autograd import BatchNormNCHWFunction
        return BatchNormNCHWFunction.apply(x_nc, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
    return F.batch_norm(x_nc, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, bn.momentum, bn.eps)   # H*W % 4 != 0


def _bn_last(x, bn):
    """(T, B, ..., C) channel-last: the reference permutes channels to dim 2, flattens (T, B) and applies BatchNorm2d - the
    same statistics are the column statistics of the (rows, C) matrix, taken in place by the HIP kernels (no permute copies)."""
    from .autograd import BatchNormLastFunction
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return BatchNormLastFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)


def _bn_ch2(x, bn):
    """(T, B, C, H, W) -> BatchNorm2d on the (T*B, C, H, W) view."""
    return _bn(x.flatten(0, 1), bn).view(x.shape)


def _conv_seq(x, conv, stride=None, padding=None, spikes=False):
    """layer.Conv2d in multi-step mode: (T, B, C, H, W) through one conv2d call on the flattened batch.  spikes=True: x is a neuron's
    output - a 3x3 / stride 1 / pad 1 convolution with 96-multiples of channels then takes its WEIGHT gradient on csrc/linear_dw.hip
    (convolution form); forward and dX stay library convolutions."""
    T, B = x.shape[:2]
    x2 = x.flatten(0, 1)
    if (spikes and CONV_DW_HIP and stride is None and padding is None and x2.is_cuda and tuple(conv.kernel_size) == (3, 3)
            and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and hip.conv3x3_dw_applicable(x2.shape[0], conv.in_channels, conv.out_channels, x2.shape[2], x2.shape[3])):
        from .autograd import Conv3x3DwFunction, Conv3x3HipFunction
        if CONV_FWD_HIP and not torch.is_autocast_enabled() and conv.in_channels % 32 == 0:
            y = Conv3x3HipFunction.apply(x2, conv.weight, conv.bias)
        else:
            y = Conv3x3DwFunction.apply(x2, conv.weight, conv.bias)
    else:
        y = F.conv2d(x2, conv.weight, conv.bias, conv.stride if stride is None else stride, conv.padding if padding is None else padding)
    return y.view(T, B, *y.shape[1:])


def _drop_path(x, p, training):
    if p <= 0.0 or not training:
        return x
    keep = 1.0 - p
    mask = torch.empty((x.shape[0],) + (1,) * (x.dim() - 1), dtype=x.dtype, device=x.device).bernoulli_(keep)
    return x * (mask / keep)


def rebin_events(x, num_bins, num_steps):
    """(B, bins, 2, H, W) -> (T, B, num_ch, H, W): time step t takes bin t of each polarity (patch embedding :1775-1784)."""
    if x.size(1) > num_bins:
        x = x[:, :num_bins]
    num_ch = num_bins * 2 // num_steps
    ev = x.permute(0, 2, 3, 4, 1)
    chans = [ev[:, i % 2, :, :, (i // 2) * num_steps:(i // 2 + 1) * num_steps] for i in range(num_ch)]
    return torch.stack(chans, 1).permute(4, 0, 1, 2, 3).contiguous()


def ms_resblock(x, rb):
    y = rb.sn1(x)
    y = _bn_ch2(_conv_seq(y, rb.conv1[0], spikes=True), rb.norm1.norm_layer)
    y = rb.sn2(y)
    y = _bn_ch2(_conv_seq(y, rb.conv2[0], spikes=True), rb.norm2.norm_layer)
    return y + x


def patch_embed(x, pe):
    x = rebin_events(x, pe.num_bins, pe.num_steps)
    y = pe.head.sn(_bn_ch2(_conv_seq(x, pe.head.conv[0]), pe.head.norm_layer.norm_layer))
    y = _bn_ch2(_conv_seq(y, pe.conv.conv[0]), pe.conv.norm_layer.norm_layer)
    for rb in pe.residual_encoding.resblocks:
        y = ms_resblock(y, rb)
    T, B = y.shape[:2]
    res = F.conv2d(y.flatten(0, 1), pe.proj.conv_res.weight, pe.proj.conv_res.bias, stride=2)
    s = pe.proj.sn(y)
    z = F.conv2d(s.flatten(0, 1), pe.proj.conv.weight, pe.proj.conv.bias, stride=2, padding=1)
    z = _bn(z, pe.proj.norm_layer) + res
    return z.view(T, B, *z.shape[1:])


def get_window_size(x_size, window_size, shift_size):
    ws, ss = list(window_size), list(shift_size)
    for i in range(3):
        if x_size[i] <= window_size[i]:
            ws[i], ss[i] = x_size[i], 0
    return tuple(ws), tuple(ss)


def qk_attention(x, attn):
    """x (T', B_, N1, C): slice list of the windows, T' = window depth.  Returns (T', B_, N1, C)."""
    Tq, B_, N1, C = x.shape
    nH = attn.num_heads
    hd = C // nH
    xs = attn.proj_sn(x)
    q = attn.sn_q(_bn_last(_linear(xs, attn.linear_q), attn.bn_q.norm_layer))
    k = _bn_last(_linear(xs, attn.linear_k), attn.bn_k.norm_layer)
    k = attn.sn_k(k + attn.positional_encoding.reshape(Tq, 1, N1, C))
    gate = attn.sn2_q.spiking_neuron
    composed = isinstance(gate, (GatedLIFNode, SLTTLIFNode))            # GLIF / SLTT-LIF gate: head sum -> the node's own Function -> * k
    if hd == 32 and Tq in (1, 2, 4) and not composed:                   # token gate, forward and backward one HIP launch each
        from .autograd import QKGateFunction
        alpha = getattr(gate.surrogate_function, "alpha", 2.0)
        if isinstance(gate, ParametricLIFNode):                          # (its `kind` stays "lif": the inference engine reads that)
            from .autograd import QKGatePLIFFunction
            e = QKGatePLIFFunction.apply(q, k, gate.k(), gate.v_threshold, gate.v_reset, gate.detach_reset, alpha)
        elif gate.kind == "psn":
            e = QKGateFunction.apply(q, k, gate.weight, gate.bias, "psn", 2.0, 0.0, None, True, alpha)
        else:
            e = QKGateFunction.apply(q, k, None, None, gate.kind, gate.tau, gate.v_threshold, gate.v_reset, gate.detach_reset, alpha)
    else:                                                               # other head widths / window depths / gates: composed expression
        a = attn.sn2_q(q.reshape(Tq, B_, N1, nH, hd).sum(-1))
        e = k * a.repeat_interleave(hd, dim=-1)
    z = e.reshape(B_, nH, Tq, N1, hd).permute(2, 0, 3, 1, 4).reshape(Tq, B_, N1, C)     # the reference's raw head reshape
    return _bn_last(_linear(z, attn.proj), attn.proj_bn.norm_layer)


_SLICE_MAPS = {}


def _slice_map(x, blk):
    """(window size, shift, int32 slice map, B_) of block `blk` on x (B, D, H, W, C): the map is built on the device, cached per shape."""
    B, D, H, W, C = x.shape
    (Wd, Wh, Ww), ss = get_window_size((D, H, W), blk.window_size, blk.shift_size)
    key = (B, D, H, W, Wd, Wh, Ww, ss, str(x.device))
    if key not in _SLICE_MAPS:
        _SLICE_MAPS[key] = hip.window_slice_map(B, D, H, W, (Wd, Wh, Ww), ss, x.device)
    return (Wd, Wh, Ww), ss, *_SLICE_MAPS[key]


def ssa(x, blk):
    """Window partition -> attention -> window reverse, both as row moves through the int32 slice map (built on the device,
    cached per shape): no materialised pad / roll / permute / crop in either direction of autograd."""
    from .autograd import WindowGatherFunction, WindowScatterFunction
    B, D, H, W, C = x.shape
    (Wd, Wh, Ww), ss, row_map, B_ = _slice_map(x, blk)
    xw = WindowGatherFunction.apply(x, row_map)                          # (Wd * B_ * Wh * Ww, C): step t' of window b' is slice t' B_ + b'
    y = qk_attention(xw.view(Wd, B_, Wh * Ww, C), blk.attn)
    return WindowScatterFunction.apply(y.reshape(-1, C), row_map, (B, D, H, W, C))


def ms_mlp(x, mlp):
    h = _bn_last(_linear(mlp.sn1(x), mlp.fc1), mlp.bn1.norm_layer)
    return _bn_last(_linear(mlp.sn2(h), mlp.fc2), mlp.bn2.norm_layer)


def ms_block(x, blk, training=True):
    x = _drop_path(ssa(x, blk), blk.drop_path_rate, training) + x
    return ms_mlp(x.permute(1, 0, 2, 3, 4).contiguous(), blk.mlp).permute(1, 0, 2, 3, 4) + x


def ms_patch_merge(x, pm):
    B, D, H, W, C = x.shape
    if H % 2 or W % 2:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], -1)
    x = pm.sn(x.permute(1, 0, 2, 3, 4).contiguous())
    return _bn_last(_linear(x, pm.reduction), pm.norm.norm_layer).permute(1, 0, 2, 3, 4)


def skip_concat_ch(x1, x2):
    dY, dX = x2.shape[-2] - x1.shape[-2], x2.shape[-1] - x1.shape[-1]
    return torch.cat([F.pad(x1, (dX // 2, dX - dX // 2, dY // 2, dY - dY // 2)), x2], dim=2)


def _flows_of_preds(preds, H, W):
    """The models' tail on the raw predictions: sum over time, nearest upsampling to (H, W) - one (B, 2, H, W) map per level."""
    flows = []
    for f in preds:
        f = f.sum(0)
        flows.append(F.interpolate(f, scale_factor=(H / f.shape[-2], W / f.shape[-1])))
    return flows


def forward_train(model, x):
    """(B, bins, 2, H, W) on the GPU -> list of flow maps (B, 2, H, W), differentiable; BN running stats are updated."""
    return _flows_of_preds(forward_train_preds(model, x), *x.shape[-2:])


def forward_train_preds(model, x):
    """`forward_train` up to the decoder levels' raw predictions: a list of (T, B, 2, h, w), coarsest first (what `flow_loss_hip` takes)."""
    if not x.is_cuda:
        raise hip.SdfError("the training path runs on the GPU only (no CPU fallback)")
    unet = model.sttmultires_unet
    sw = unet.encoders.swin3d
    y = patch_embed(x.float(), sw.patch_embed).permute(1, 0, 3, 4, 2).contiguous()          # (B, D, h, w, C)
    blocks = []
    for i, layer in enumerate(sw.layers):
        for blk in layer.swin_blocks:
            y = ms_block(y, blk, model.training)
        if i in sw.out_indices:
            blocks.append(y.permute(1, 0, 4, 2, 3).contiguous())                            # (D, B, C, h, w)
        if layer.downsample is not None:
            y = ms_patch_merge(y, layer.downsample)
    y = blocks[-1]
    for rb in unet.resblocks:
        y = ms_resblock(y, rb)
    preds, E = [], len(blocks)
    for i in range(E):
        y = skip_concat_ch(y, blocks[E - i - 1])
        if i > 0:
            y = skip_concat_ch(preds[-1], y)
        dec, pr = unet.decoders[i], unet.preds[i]
        s = dec.sn(y.contiguous())
        T, B = s.shape[:2]
        dc = dec.deconv[0]
        z = F.conv_transpose2d(s.flatten(0, 1), dc.weight, dc.bias, stride=2, padding=dc.kernel_size[0] // 2, output_padding=1)
        y = _bn_ch2(z.view(T, B, *z.shape[1:]), dec.norm_layer.norm_layer)
        preds.append(_conv_seq(pr.sn(y), pr.conv[0], padding=0))
    return preds


# ---------------------------------------------------------------------------------------------- SEW family (SpikingformerFlowNet)
# The stream between SEW blocks carries SUMS of spikes (reference Spiking_STSwinNet.py:254-311).  Every layer that reads it (q / k / v,
# fc1, the merge reduction, the res-block's first convolution, the decoders) and the real-valued attention output (proj) take library
# products: the hand-written spike products keep the top 16 bits of the activation and would truncate them.  Only the layers a neuron
# feeds (fc2, the res-block's second convolution) take the spike products.
def sew_attention_core_torch(q, k, v, scale, bias, mask, nH):
    """The core of `autograd.WinAttnSewFunction` as a torch composition (reference Spiking_swin_transformer3D.py:320-363), fp32: the A/B
    path of SDF_SEW_ATTN_BWD=0.  It keeps the (B_, nH, N, N) scores for autograd."""
    Tq, B_, N1, Cc = q.shape
    N, hd = Tq * N1, Cc // nH
    with torch.autocast("cuda", enabled=False):
        qh, kh, vh = (t.float().reshape(B_, nH, N, hd) for t in (q, k, v))
        a = (qh * scale.float().view(1, nH, 1, 1)) @ kh.transpose(-2, -1) + bias.float().unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            a = (a.view(B_ // nW, nW, nH, N, N) + mask.float().view(1, nW, 1, N, N)).view(B_, nH, N, N)
        o = a @ vh
    return o.reshape(B_, nH, Tq, N1, hd).permute(2, 0, 3, 1, 4).reshape(Tq, B_, N1, Cc)


def sew_attention(xw, attn, mask):
    """`Spiking_BN_WindowAttention3D.forward` in training (reference :300-370): xw (T', B_, N1, C) window slices of the SEW stream ->
    (T', B_, N1, C) spikes.  q / k / v = SN(BN(Linear)); the core is `autograd.WinAttnSewFunction` (HIP both ways; SDF_SEW_ATTN_BWD=0:
    the torch composition); the relative-position bias is the table gathered under autograd; proj (with bias) -> BN -> SN."""
    Tq, B_, N1, Cc = xw.shape
    nH, N = attn.num_heads, Tq * N1
    hip.check_attn_bwd_window(N, "SDF_SEW_ATTN_BWD")
    q, k, v = (getattr(attn, f"sn_{n}")(_bn_last(_linear(xw, getattr(attn, f"linear_{n}"), spikes=False), getattr(attn, f"bn_{n}").norm_layer))
               for n in ("q", "k", "v"))
    bias = attn.relative_position_bias_table[attn.relative_position_index[:N, :N].reshape(-1)].reshape(N, N, nH).permute(2, 0, 1)
    scale = torch.full((nH,), float(attn.scale), dtype=torch.float32, device=xw.device)
    if hip.sw("SDF_SEW_ATTN_BWD", "1") == "0":
        z = sew_attention_core_torch(q, k, v, scale, bias, mask, nH)
    else:
        from .autograd import WinAttnSewFunction
        z = WinAttnSewFunction.apply(q, k, v, bias.float(), scale, mask, nH)
    return attn.proj_sn(_bn_last(_linear(z, attn.proj, spikes=False), attn.proj_bn.norm_layer))


def sew_ssa(x, blk):
    """`Spiking_SwinTransformerBlock3D.SSA` around the SEW attention (Spiking_swin_transformer3D.py:781-821) through the slice map; the
    shift mask of the padded grid is passed whenever the block is shifted (:799-801, layer forward :1070-1076)."""
    from .autograd import WindowGatherFunction, WindowScatterFunction
    from .STSwinNet.swin_transformer3D_v2 import compute_mask
    B, D, H, W, C = x.shape
    ws, ss, row_map, B_ = _slice_map(x, blk)
    mask = None
    if any(s > 0 for s in ss):
        mask = compute_mask(-(-D // ws[0]) * ws[0], -(-H // ws[1]) * ws[1], -(-W // ws[2]) * ws[2], ws, ss, x.device).contiguous()
    xw = WindowGatherFunction.apply(x, row_map)
    y = sew_attention(xw.view(ws[0], B_, ws[1] * ws[2], C), blk.attn, mask)
    return WindowScatterFunction.apply(y.reshape(-1, C), row_map, (B, D, H, W, C))


def sew_mlp(x, mlp):
    """`Spiking_Mlp.forward` (:147-162): fc1 -> BN -> SN -> fc2 -> BN -> SN on (T, B, H, W, C)."""
    h = mlp.sn1(_bn_last(_linear(x, mlp.fc1, spikes=False), mlp.bn1.norm_layer))
    return mlp.sn2(_bn_last(_linear(h, mlp.fc2), mlp.bn2.norm_layer))


def sew_block(x, blk, training=True):
    """`Spiking_SwinTransformerBlock3D.forward`, cnf ADD (:824-847): DropPath on the SSA branch, as the MS block."""
    x = _drop_path(sew_ssa(x, blk), blk.drop_path_rate, training) + x
    return sew_mlp(x.permute(1, 0, 2, 3, 4).contiguous(), blk.mlp).permute(1, 0, 2, 3, 4) + x


def sew_patch_merge(x, pm):
    """`SpikingPatchMerging.forward` (:914-934): 2x2 gather -> Linear -> BN -> SN."""
    B, D, H, W, C = x.shape
    if H % 2 or W % 2:
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], -1)
    y = _bn_last(_linear(x.permute(1, 0, 2, 3, 4).contiguous(), pm.reduction, spikes=False), pm.norm.norm_layer)
    return pm.sn(y).permute(1, 0, 2, 3, 4)


def sew_resblock(x, rb):
    """`SEWResBlock.forward`, connect ADD (Spiking_modules.py:852-878): conv-BN-SN-conv-BN-SN + identity on (T, B, C, H, W)."""
    y = rb.sn1(_bn_ch2(_conv_seq(x, rb.conv1[0]), rb.norm1.norm_layer))
    y = rb.sn2(_bn_ch2(_conv_seq(y, rb.conv2[0], spikes=True), rb.norm2.norm_layer))
    return y + x


def forward_train_sew(model, x):
    """`SpikingformerFlowNet.forward` in train mode (Spiking_STSwinNet.py:278-305, :161-182): (B, bins, 2, H, W) on the GPU -> list of
    flow maps (B, 2, H, W), differentiable; BN running statistics are updated.  Same patch embedding as the MS models; SEW blocks,
    SEW patch merging, SEW res-blocks, decoders ConvT 3x3 s2 -> BN -> SN (no neuron in front), plain 1x1 predictions."""
    return _flows_of_preds(forward_train_sew_preds(model, x), *x.shape[-2:])


def forward_train_sew_preds(model, x):
    """`forward_train_sew` up to the decoder levels' raw predictions: a list of (T, B, 2, h, w), coarsest first."""
    if not x.is_cuda:
        raise hip.SdfError("the training path runs on the GPU only (no CPU fallback)")
    unet = model.sttmultires_unet
    sw = unet.encoders.swin3d
    ws = sw.layers[0].swin_blocks[0].attn.window_size
    hip.check_attn_bwd_window(ws[0] * ws[1] * ws[2], "SDF_SEW_ATTN_BWD")                    # (before the first launch, not in block 0)
    y = patch_embed(x.float(), sw.patch_embed).permute(1, 0, 3, 4, 2).contiguous()          # (B, D, h, w, C)
    blocks = []
    for i, layer in enumerate(sw.layers):
        for blk in layer.swin_blocks:
            y = sew_block(y, blk, model.training)
        if i in sw.out_indices:
            blocks.append(y.permute(1, 0, 4, 2, 3).contiguous())                            # (D, B, C, h, w)
        if layer.downsample is not None:
            y = sew_patch_merge(y, layer.downsample)
    y = blocks[-1]
    for rb in unet.resblocks:
        y = sew_resblock(y, rb)
    preds, E = [], len(blocks)
    for i in range(E):
        y = skip_concat_ch(y, blocks[E - i - 1])
        if i > 0:
            y = skip_concat_ch(preds[-1], y)
        dec, pr = unet.decoders[i], unet.preds[i]
        T, B = y.shape[:2]
        dc = dec.deconv[0]
        z = F.conv_transpose2d(y.flatten(0, 1), dc.weight, dc.bias, stride=2, padding=dc.kernel_size[0] // 2, output_padding=1)
        y = dec.sn(_bn_ch2(z.view(T, B, *z.shape[1:]), dec.norm_layer.norm_layer))
        preds.append(_conv_seq(y, pr.conv[0], padding=0))
    return preds


# ---------------------------------------------------------------------------------------------- loss, step, all-reduce
def flow_loss_supervised(pred_list, gt_flow, mask, flow_scaling=1.0, lambda_mod=1.0, n_valid=None):
    """Mean over predictions and samples of sum(EPE * mask) / (number of valid pixels) (reference loss/flow_supervised.py:85-102).
    `n_valid` replaces the local count when the batch is sharded over ranks (see `global_valid_count`)."""
    n = torch.sum(mask) if n_valid is None else n_valid
    cur = 0.0
    for pred in pred_list:
        flow = pred * flow_scaling
        err = torch.sqrt((flow - gt_flow).pow(2).sum(1) + 1e-8).view(flow.shape[0], -1) * mask.reshape(flow.shape[0], -1)
        cur = cur + lambda_mod * (torch.sum(err, dim=1) / (n + 1e-9))
    return torch.mean(cur / len(pred_list))


def flow_loss_hip(preds, label, mask, flow_scaling=1.0, lambda_mod=1.0, n_valid=None):
    """`flow_loss_supervised` on the RAW predictions `forward_train_preds` returns - a list of (T, B, 2, h, w), each a factor 1, 2, 4, 8
    or 16 below the label - in two launches of csrc/flow_loss.hip (hip.flow_loss): the sum over time, the nearest upsampling and the
    loss in one pass over the frame, the gradient delivered at each level's own resolution (autograd.FlowLossFunction).  Opt-in
    (`train_step(head="hip")`); the values agree with the torch head to rounding, not bit for bit.  Under torch.no_grad(), or when no
    prediction needs a gradient, the loss alone is computed."""
    from .autograd import FlowLossFunction
    n = torch.sum(mask) if n_valid is None else n_valid
    n, label, mask = n.float().reshape(1), label.float(), mask.float()
    if not (torch.is_grad_enabled() and any(p.requires_grad for p in preds)):
        return hip.flow_loss(preds, label, mask, n, flow_scaling, lambda_mod, grads=False)[0]
    return FlowLossFunction.apply(label, mask, n, float(flow_scaling), float(lambda_mod), *preds)


def global_valid_count(mask, dist=None, world=1):
    """Valid pixels of the GLOBAL batch.  The reference trains under nn.DataParallel: the replicas' outputs are gathered and
    the loss is taken on the whole batch, so every sample's error is divided by the valid-pixel count of the whole batch
    (loss/flow_supervised.py:90, train_flow_parallel_supervised_SNN.py:139-143, :306-308).  With one process per GPU the
    count is summed over the ranks (one scalar all-reduce, issued before the backward pass); together with the mean over
    ranks of the gradients this reproduces the gathered-batch gradient exactly - normalising by the local count instead
    makes the gradient ~world times larger."""
    n = torch.sum(mask).float()
    if dist is not None and world > 1:
        dist.all_reduce(n, op=dist.ReduceOp.SUM)
    return n


class GradientBuckets:
    """Flat fp32 gradient buckets for the data-parallel step: the parameters' `.grad` are VIEWS into a few large
    contiguous buffers (default 64 MiB - ring all-reduce over xGMI is per-link bound, few large messages beat many small
    ones; the whole en4 model is 220 MB = 4 buckets), so a bucket's all-reduce is one collective with no packing copies.

    Overlap with backward: every parameter carries a post-accumulate-grad hook; when the last parameter of a bucket has
    its gradient the bucket's all-reduce is launched asynchronously right there, inside `loss.backward()` (buckets are
    filled in reverse parameter order = the order backward produces gradients, so the first collective leaves while most
    of the backward pass is still to run).  `finish()` launches whatever is left - buckets holding a parameter that
    received no gradient this step - waits for all, divides by world, and hands parameters that never received a
    gradient to the optimiser as `.grad = None` (the reference leaves them None: no weight decay / moment updates on
    the dead attn_sn weights).  Every rank launches the same collectives in the same order: completion order is a
    property of the autograd graph, the left-overs go in bucket order."""

    def __init__(self, params, bucket_bytes=64 << 20):
        self.params = [p for p in params if p.requires_grad]
        self.buckets, cur, cur_n = [], [], 0
        for p in reversed(self.params):                                # backward produces gradients last layer first
            if cur and (cur_n + p.numel()) * 4 > bucket_bytes:
                self.buckets.append(cur)
                cur, cur_n = [], 0
            cur.append(p)
            cur_n += p.numel()
        if cur:
            self.buckets.append(cur)
        self.flat, self._views, self._bucket_of = [], {}, {}
        for bi, b in enumerate(self.buckets):
            buf = torch.zeros(sum(p.numel() for p in b), dtype=torch.float32, device=b[0].device)
            off = 0
            for p in b:
                self._views[p] = buf[off:off + p.numel()].view_as(p)
                self._bucket_of[p] = bi
                p.grad = self._views[p]
                off += p.numel()
                p.register_post_accumulate_grad_hook(self._ready)
            self.flat.append(buf)
        self._dist, self._world = None, 1
        self._pending = [len(b) for b in self.buckets]
        self._seen, self._works, self._launched = set(), [], set()
        self._seen_sum = set()                                          # ... over the micro-steps of a running sum (begin(zero=False))
        self.accumulating = False                                       # train_step: the buckets hold a running sum the next call keeps
        self.log = []                                                   # (event, bucket index, hooks fired so far): test hook
        self.stats = None                                               # BucketStats, made by its first user (bucket_stats)

    def zero(self):
        for buf in self.flat:
            buf.zero_()

    def begin(self, dist=None, world=1, zero=True):
        """Start of a step: zero the buckets, re-attach the `.grad` views, arm the hooks.  `zero=False` (gradient accumulation) keeps the
        running sum: the views are re-attached and the hooks re-armed, and a parameter counts as having a gradient if any
        micro-step since the last zeroing gave it one."""
        if zero:
            self.zero()
            self._seen_sum = set()
        if self.stats is not None:
            self.stats.valid = self.stats.clipped = False
        for p, v in self._views.items():
            p.grad = v
        self._dist, self._world = (dist, world) if (dist is not None and world > 1) else (None, 1)
        self._pending = [len(b) for b in self.buckets]
        self._seen, self._works, self._launched, self.log = set(), [], set(), []

    def _launch(self, bi):
        self._launched.add(bi)
        self.log.append(("all_reduce", bi, len(self._seen)))
        if self._dist is not None:
            self._works.append(self._dist.all_reduce(self.flat[bi], op=self._dist.ReduceOp.SUM, async_op=True))

    def _ready(self, p):
        if id(p) in self._seen:
            return
        self._seen.add(id(p))
        if p.grad is not self._views[p]:                                # autograd replaced the view (first accumulation into None)
            self._views[p].copy_(p.grad)
            p.grad = self._views[p]
        bi = self._bucket_of[p]
        self._pending[bi] -= 1
        if self._pending[bi] == 0:
            self._launch(bi)

    def finish(self):
        """After backward: remaining buckets, wait, average, `.grad = None` for parameters without a gradient."""
        for bi in range(len(self.buckets)):
            if bi not in self._launched:
                self._launch(bi)
        for w in self._works:
            w.wait()
        if self._dist is not None:
            for buf in self.flat:
                buf.div_(self._world)
        self._seen_sum |= self._seen
        for p in self.params:
            if id(p) not in self._seen_sum:
                p.grad = None
        self._works = []

    def all_reduce(self, dist=None, world=1):
        """Non-overlapped form (gradients already complete): sum over ranks / world, one collective per bucket."""
        if dist is None or world <= 1:
            return
        works = [dist.all_reduce(buf, op=dist.ReduceOp.SUM, async_op=True) for buf in self.flat]
        for w in works:
            w.wait()
        for buf in self.flat:
            buf.div_(world)


# ---------------------------------------------------------------------------------------------- the step's tail on the buckets
class BucketStats:
    """Per-parameter gradient statistics of a GradientBuckets on the GPU (csrc/grad_step.hip): one (offset, length) table per bucket,
    ONE statistics table for all of them - row r is parameter `params[r]`, bucket after bucket, hip.GRAD_STATS_FIELDS - and behind it,
    in the same allocation, the clip record [total norm, non-finite count] and the fp32 clip coefficient, so that one read-back
    fetches everything.  `compute()` is two launches per bucket, `clip()` one more; nothing waits for the host."""

    def __init__(self, buckets):
        self.params = [p for b in buckets.buckets for p in b]
        if not self.params:
            raise ValueError("BucketStats: the buckets hold no parameter")
        self.flat, self.segments, self.row0, self.row_of = buckets.flat, [], [], {}
        for flat, b in zip(buckets.flat, buckets.buckets):
            pairs = []
            for p in b:
                v = buckets._views[p]
                self.row_of[p] = len(self.row_of)
                pairs.append(((v.data_ptr() - flat.data_ptr()) // 4, v.numel()))
            self.row0.append(len(self.row_of) - len(b))
            self.segments.append(hip.GradSegments(pairs, flat.device))
        n, dev = len(self.params), buckets.flat[0].device
        self._buf = torch.zeros(n * 5 + 3, dtype=torch.float64, device=dev)
        self.table, self.record = self._buf[:n * 5].view(n, 5), self._buf[n * 5:n * 5 + 2]
        self.coef = self._buf[n * 5 + 2:].view(torch.float32)[:1]
        self.mask, self._mask_key = torch.ones(n, dtype=torch.uint8, device=dev), None
        self.lengths = [p.numel() for p in self.params]
        self.valid = self.clipped = False
        self.scaled = False                                             # the last clip() ran with a loss scaler

    def compute(self):
        for flat, seg, row0 in zip(self.flat, self.segments, self.row0):
            hip.grad_stats(flat, seg, self.table, row0)
        self.valid, self.clipped = True, False

    def clip(self, max_norm, active=None, scaler=None, clip_unscaled=False):
        """The clip coefficient over the rows with active[r] (None: all) into `coef`; max_norm None = inf: coef 1, the norm is recorded.
        With a `scaler` (LossScaler) the same launch also gives the verdict on the step and updates the scale (hip.grad_clip_scale_coef)."""
        key = None if active is None else bytes(bytearray(int(bool(a)) for a in active))           # (a few hundred rows)
        if key != self._mask_key:
            host = torch.ones(len(self.params), dtype=torch.uint8) if key is None else torch.frombuffer(bytearray(key), dtype=torch.uint8)
            self.mask.copy_(host.pin_memory(), non_blocking=True)
            self._mask_key = key
        if scaler is None:
            hip.grad_clip_coef(self.table, float("inf") if max_norm is None else max_norm, self.mask, self.coef, self.record)
        else:
            hip.grad_clip_scale_coef(self.table, float("inf") if max_norm is None else max_norm, scaler.state, scaler.growth_factor,
                                     scaler.backoff_factor, scaler.growth_interval, self.mask, self.coef, self.record,
                                     clip_unscaled=clip_unscaled, update=scaler.enabled)
        self.clipped, self.scaled = True, scaler is not None

    def scale_inplace(self):
        """flat *= coef over the rows of the last clip(): clip_grad_norm_'s in-place pass (one launch per bucket)."""
        for flat, seg, row0 in zip(self.flat, self.segments, self.row0):
            hip.grad_scale(flat, seg, self.coef, self.mask[row0:row0 + seg.n])

    def read(self):
        """ONE read-back: (table (n, 5) float64 numpy, [total norm, non-finite count], coef)."""
        host = self._buf.cpu()
        n = len(self.params)
        return host[:n * 5].view(n, 5).numpy(), host[n * 5:n * 5 + 2].tolist(), float(host[n * 5 + 2:].view(torch.float32)[0])


def bucket_stats(buckets):
    """The buckets' BucketStats, made at the first call."""
    if buckets.stats is None:
        buckets.stats = BucketStats(buckets)
    return buckets.stats


def grad_stats_record(named_grads, coef=1.0):
    """numpy restatement (float64) of the statistics kernel and of get_grads' arithmetic: {name: gradient array or None} ->
    ({name_mean, name_min, name_max}, rows {name: (sum_abs, sum_sq, min_abs, max_abs, nonfinite)}).  Non-finite elements are counted and
    left out of the sums and extremes; a parameter holding one records NaN.  `coef` scales to the post-clip values."""
    import math
    import numpy as np
    record, rows = {}, {}
    for name, g in named_grads.items():
        a = np.abs(np.asarray(g, dtype=np.float32).reshape(-1)).astype(np.float64)
        fin = a[np.isfinite(a)]
        bad = a.size - fin.size
        rows[name] = (math.fsum(fin), math.fsum(fin * fin), float(fin.min()) if fin.size else math.inf,
                      float(fin.max()) if fin.size else 0.0, float(bad))
        nan = bad > 0
        record[f"{name}_mean"] = math.nan if nan else rows[name][0] / a.size * coef
        record[f"{name}_min"] = math.nan if nan else rows[name][2] * coef
        record[f"{name}_max"] = math.nan if nan else rows[name][3] * coef
    return record, rows


def clip_coef_restatement(sum_sq, max_norm):
    """(coef, total) of sdf_grad_clip_coef in float64: clip_grad_norm_'s formula on the per-parameter sums of squares."""
    import math
    total = math.sqrt(math.fsum(sum_sq))
    return min(1.0, float(max_norm) / (total + 1e-6)), total


def adamw_scalars(step, lr, betas, eps, weight_decay):
    """The scalars of AdamW's step number `step` as Python doubles, formed as torch.optim.AdamW(foreach=False) forms them:
    (decay, w1, beta2, w2, neg_step_size, bc2_sqrt, eps)."""
    b1, b2 = betas
    return (1 - lr * weight_decay, 1 - b1, b2, 1 - b2, -(lr / (1 - b1 ** step)), (1 - b2 ** step) ** 0.5, eps)


def adamw_restatement(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, coef=1.0):
    """numpy restatement (float64 throughout) of one sdf_adamw_step on one parameter: returns the new (p, m, v).  `step` is the number
    of THIS step (1 for the first); `coef` the clip coefficient the gradient is multiplied by."""
    import numpy as np
    decay, w1, beta2, w2, nstep, bc2s, eps = adamw_scalars(step, lr, betas, eps, weight_decay)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = g * float(coef)
    p = p * decay
    m = m + w1 * (g - m)
    v = v * beta2 + w2 * g * g
    return p + nstep * m / (np.sqrt(v) / bc2s + eps), m, v


def loss_scale_restatement(scale, growth_tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """numpy restatement of the scale update of sdf_grad_clip_scale_coef - torch's _amp_update_scale_ with the scale and both factors as
    fp32: (scale, growth_tracker) after a step whose gradients were (`found_inf`) or were not all finite."""
    import numpy as np
    scale = np.float32(scale)
    if found_inf:
        return float(scale * np.float32(backoff_factor)), 0
    if growth_tracker + 1 == growth_interval:
        with np.errstate(over="ignore"):
            grown = scale * np.float32(growth_factor)
        return float(grown if np.isfinite(grown) else scale), 0
    return float(scale), growth_tracker + 1


class LossScaler:
    """torch.amp.GradScaler's dynamic loss scale as a device-resident SdfLossScaleState (csrc/grad_step.hip): `scale(loss)` multiplies
    by the device scalar, `BucketAdamW.step(..., scaler=this)` finds non-finite gradients, skips the update, divides the scale out
    and grows or backs the scale off - all in the kernels, without the host waiting for the verdict.  `get_scale()` and `skipped`
    (steps skipped since construction) are host reads.  `state_dict()` / `load_state_dict()` carry exactly GradScaler's keys and
    interchange with it.  `enabled=False`: the scale is 1 and stays 1; only the skip of a non-finite step remains."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True, device="cuda"):
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1 and init_scale > 0.0):
            raise ValueError(f"LossScaler: init_scale {init_scale}, growth_factor {growth_factor} (> 1), backoff_factor {backoff_factor} "
                             f"(in (0, 1)), growth_interval {growth_interval} (>= 1)")
        self.enabled = bool(enabled)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.device = torch.device(device)
        self._pending = []                                              # reconciliations of steps whose verdict the host has not read
        self._set(float(init_scale) if self.enabled else 1.0, 0)

    def _set(self, scale, tracker, skipped=0):
        self.state = hip.loss_scale_state(scale, tracker, self.device)
        self._views = hip.loss_scale_views(self.state)
        self._views["skipped"].fill_(int(skipped))
        self._scale = self._views["scale"][0]                           # a 0-dim view: what a loss is multiplied by

    def scale(self, loss):
        """loss * scale, the scale read on the device (no synchronisation); the loss itself when not enabled."""
        return loss * self._scale if self.enabled else loss

    def reconcile(self):
        """Read the verdicts of the steps taken so far (BucketAdamW rolls the host's step counts of a skipped one back)."""
        pending, self._pending = self._pending, []
        for fn in pending:
            fn()

    def get_scale(self):
        return float(self._scale)

    @property
    def skipped(self):
        self.reconcile()
        return int(self._views["skipped"])

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys and values; {} when not enabled, as GradScaler's."""
        if not self.enabled:
            return {}
        host = hip.loss_scale_read(self.state)
        return {"scale": host["scale"], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": host["growth_tracker"]}

    def load_state_dict(self, state_dict):
        if not self.enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("LossScaler.load_state_dict: the state dict is empty - it was saved from a disabled scaler")
        self.reconcile()
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval = int(state_dict["growth_interval"])
        self._set(float(state_dict["scale"]), int(state_dict["_growth_tracker"]), int(self._views["skipped"]))


class BucketAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay; no amsgrad, no maximize, one param group) on a GradientBuckets' flat buffers: the
    moments are two flat buffers per bucket with the buckets' layout - `state[p]["exp_avg"]` / `["exp_avg_sq"]` are views into them,
    `state[p]["step"]` torch's float32 CPU scalar - and `step(clip_grad)` is gradient statistics -> clip coefficient -> update on
    csrc/grad_step.hip, on the current stream, without a host synchronisation: the update reads the coefficient from device memory.
    The gradients themselves are NOT scaled in place (clip_grad_norm_ does); `get_grads` scales what it reports.  A parameter whose
    `.grad` is None (GradientBuckets.finish) is not touched - not its value, its moments or its step count - as in torch.
    `state_dict()` / `load_state_dict()` interchange with torch.optim.AdamW over the same parameters.
    `step(clip_grad, scaler=LossScaler)`: the same number of launches, the coefficient kernel also deciding whether the step is off
    (a non-finite gradient) and the update obeying it: a skipped step writes no parameter and no moment.  The host does not wait for
    that verdict: it counts the step, copies the verdict into a pinned slot behind the launches and reads the slot at the start of
    the next step() (or in state_dict() / LossScaler.skipped), rolling the counts of a skipped step back before they are used again.
    The clip bounds the STILL-SCALED norm unless `clip_unscaled` (a loop that calls clip_grad_norm_ without scaler.unscale_ does the
    former)."""

    def __init__(self, buckets, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if not isinstance(buckets, GradientBuckets):
            raise TypeError("BucketAdamW(buckets, ...): the first argument is the model's GradientBuckets")
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and 0.0 <= weight_decay):
            raise ValueError(f"BucketAdamW: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        for p in buckets.params:
            if not (p.dtype == torch.float32 and p.is_contiguous() and p.numel() > 0):
                raise hip.SdfError("BucketAdamW: parameters are non-empty contiguous fp32 tensors")
        # (torch.optim.AdamW's group keys, so that a state_dict of this class loads into it; only the first four are options here)
        super().__init__(buckets.params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                              foreach=None, capturable=False, differentiable=False, fused=None,
                                              decoupled_weight_decay=True))
        self.buckets, self.stats = buckets, bucket_stats(buckets)
        self.exp_avg = [torch.zeros_like(f) for f in buckets.flat]
        self.exp_avg_sq = [torch.zeros_like(f) for f in buckets.flat]
        self._rows = hip.adamw_rows(len(self.stats.params))
        self._rows_dev = torch.zeros(self._rows.nbytes, dtype=torch.uint8, device=buckets.flat[0].device)
        self._slot = self._event = None
        self._verdict = None                                            # (pinned found_inf, event, rows counted) of a scaled step not yet read
        self._views = {}
        for bi, (b, seg) in enumerate(zip(buckets.buckets, self.stats.segments)):
            for p, (off, n) in zip(b, seg.host.tolist()):
                r = self.stats.row_of[p]
                self._rows["offset"][r], self._rows["length"][r] = off, n
                self._views[p] = (self.exp_avg[bi][off:off + n].view_as(p), self.exp_avg_sq[bi][off:off + n].view_as(p))
        self._attach({})

    def _attach(self, steps):
        """state[p] = torch's AdamW state over the flat views; `steps`: {p: step tensor to keep}."""
        import numpy as np
        for p, (m, v) in self._views.items():
            step = steps.get(p)
            self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32) if step is None else step, "exp_avg": m, "exp_avg_sq": v}
        self._step_t = [self.state[p]["step"] for p in self.stats.params]                   # row order
        self._k = np.array([float(t) for t in self._step_t], dtype=np.float64)              # their values, kept in lockstep

    def load_state_dict(self, state_dict):
        """torch's loading, then the loaded moments are copied INTO the flat views (which stay the state); a parameter the loaded
        state does not know starts from zero."""
        self._reconcile()
        super().load_state_dict(state_dict)
        if len(self.param_groups) != 1:
            raise ValueError("BucketAdamW: one param group")
        steps = {}
        for p, (m, v) in self._views.items():
            st = self.state.get(p, {})
            if "exp_avg" in st:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps[p] = torch.as_tensor(st["step"]).detach().to("cpu", torch.float32).reshape(()).clone()
            else:
                m.zero_()
                v.zero_()
        self._attach(steps)

    def _reconcile(self):
        """The verdict of the last scaled step, if the host has not read it yet: a skipped step did not happen - its rows' counts go back."""
        if self._verdict is None:
            return
        (slot, event, act), self._verdict = self._verdict, None
        event.synchronize()
        if slot.numpy()[0] != 0:
            torch._foreach_sub_([t for t, a in zip(self._step_t, act) if a], 1)
            self._k[act] -= 1

    def state_dict(self):
        self._reconcile()
        return super().state_dict()

    @torch.no_grad()
    def step(self, clip_grad=None, closure=None, scaler=None, clip_unscaled=False):
        import numpy as np
        if scaler is not None and not (isinstance(scaler, LossScaler) and scaler.state.is_cuda):
            raise hip.SdfError("BucketAdamW.step: scaler is a train.LossScaler whose state lives on the GPU (no CPU fallback)")
        self._reconcile()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise NotImplementedError("BucketAdamW: amsgrad and maximize are not built")
        lr, betas, eps, wd = float(g["lr"]), g["betas"], g["eps"], g["weight_decay"]
        st, rows = self.stats, self._rows
        act = np.fromiter((p.grad is not None for p in st.params), dtype=bool, count=len(st.params))
        st.compute()
        st.clip(clip_grad, act, scaler, clip_unscaled)
        if not act.any():
            return loss
        updated = [p for p, a in zip(st.params, act) if a]
        torch._foreach_add_([t for t, a in zip(self._step_t, act) if a], 1)
        self._k[act] += 1
        rows["active"][:] = act
        rows["param"][:] = [p.data_ptr() for p in st.params]
        for k in np.unique(self._k[act]):                                                  # (one value, unless parameters joined late)
            sel = act & (self._k == k)
            for name, val in zip(("decay", "w1", "beta2", "w2", "neg_step_size", "bc2_sqrt", "eps"), adamw_scalars(float(k), lr, betas, eps, wd)):
                rows[name][sel] = val
        # (a fresh pinned block per step: the host allocator holds it back until the copy has run, so nothing waits here)
        self._rows_dev.copy_(torch.from_numpy(rows.view("uint8")).pin_memory(), non_blocking=True)
        for bi, n in enumerate(len(b) for b in self.buckets.buckets):
            r0 = st.row0[bi]
            if not act[r0:r0 + n].any():
                continue
            if scaler is None:
                hip.adamw_step(self.buckets.flat[bi], self.exp_avg[bi], self.exp_avg_sq[bi], rows[r0:r0 + n],
                               self._rows_dev[r0 * rows.itemsize:(r0 + n) * rows.itemsize], st.coef)
            else:
                hip.adamw_step_scaled(self.buckets.flat[bi], self.exp_avg[bi], self.exp_avg_sq[bi], rows[r0:r0 + n], scaler.state,
                                      self._rows_dev[r0 * rows.itemsize:(r0 + n) * rows.itemsize], st.coef)
        if scaler is not None:                                          # the verdict follows the launches; nobody waits for it here
            if self._slot is None:
                self._slot, self._event = torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event()
            self._slot.copy_(scaler._views["found_inf"], non_blocking=True)
            self._event.record()
            self._verdict = (self._slot, self._event, act)
            if self._reconcile not in scaler._pending:
                scaler._pending.append(self._reconcile)
        # the kernel wrote through raw pointers: move the version counters, which the packed inference weights are keyed on
        torch.autograd.graph.increment_version(updated)
        return loss


def get_grads(model, buckets, coef=None, missing="skip", unscale=False, scaler=None):
    """The reference's `vis.store_grads` record (utils/gradients.py get_grads, taken after the clip): {name}_mean / _min / _max of
    |grad| of every `requires_grad` parameter with "weight" in its name, from the buckets' statistics table with ONE read-back
    instead of three `.item()` per parameter.  The statistics are those of this step (computed here unless BucketAdamW.step already
    did).  `coef`: what the clip multiplied the gradients by - None: the coefficient of this step's BucketAdamW.step, 1 without one.
    A parameter holding a non-finite gradient records NaN.  A parameter without a gradient: `missing="skip"` leaves it out,
    "raise" is the reference's AttributeError.  Under a loss scaler the record is, as the reference's, of the STILL-SCALED gradients;
    `unscale=True` with the `scaler` divides the scale these gradients carry out (one more host read)."""
    import math
    if missing not in ("skip", "raise"):
        raise ValueError('get_grads: missing is "skip" or "raise"')
    if unscale and scaler is None:
        raise ValueError("get_grads: unscale=True divides by a loss scale - pass scaler=")
    st = bucket_stats(buckets)
    if not st.valid:
        st.compute()
    table, _, dev_coef = st.read()
    c = float(coef) if coef is not None else dev_coef if st.clipped else 1.0
    if unscale:                                                         # (a scaled clip has moved `scale` on; it left the reciprocal of the old one)
        ls = hip.loss_scale_read(scaler.state)
        c *= ls["inv_scale"] if st.scaled else 1.0 / ls["scale"]
    record = {}
    for name, p in model.named_parameters():
        if not (p.requires_grad and "weight" in name):
            continue
        if p.grad is None or p not in st.row_of:
            if missing == "raise":
                raise AttributeError(f"{name} grad error: gradient returns None")
            continue
        r = st.row_of[p]
        sum_abs, _, mn, mx, bad = table[r]
        nan = bad > 0
        record[f"{name}_mean"] = math.nan if nan else float(sum_abs) / st.lengths[r] * c
        record[f"{name}_min"] = math.nan if nan else float(mn) * c
        record[f"{name}_max"] = math.nan if nan else float(mx) * c
    return record


def save_grads_csv(records, path):
    """The reference's save_csv(grads_w, "grads_w.csv") without pandas: a header (an empty index cell, then the keys of the first
    record) and one row per record, index first; appended WITHOUT a header when the file exists."""
    import csv
    if not records:
        return
    new = not os.path.isfile(path)
    keys = list(records[0])
    with open(path, "a", newline="") as f:
        w = csv.writer(f)
        if new:
            w.writerow([""] + keys)
        for i, rec in enumerate(records):
            w.writerow([i] + [repr(float(rec[k])) if k in rec else "" for k in keys])


def train_step(model, optimizer, chunk, label, mask, buckets=None, dist=None, world=1, clip_grad=100.0, flow_scaling=1.0,
               lambda_mod=1.0, amp=False, forward_fn=None, grads_out=None, scaler=None, num_acc=1, step_now=True, clip_unscaled=False,
               head="torch"):
    """One step of train_flow_parallel_supervised_SNN.py's loop body (:233-336) on this rank's shard of the batch; returns the
    loss tensor (this rank's samples' mean of err / n_global; the mean over ranks is the gathered-batch loss).
    `amp`: the reference trains under `torch.cuda.amp.autocast` with fp16 + GradScaler (`optimizer.use_amp: true`,
    :248, :314-331); here the same regions run under bf16 autocast (no scaler needed) - spikes are exact in bf16, the
    membranes / neuron kernels, BatchNorm statistics, the loss and the optimiser stay fp32.
    An STTFlowNet (the ANN family, `clip_grad=None` as its config has it) trains through its own train-mode forward,
    `model(chunk, None)["flow"]`, in fp32; a SpikingformerFlowNet (the SEW family) through `forward_train_sew`.
    `forward_fn(model, chunk) -> flows` replaces the HIP train-mode forward (the CPU dry run of the N > 1 plumbing, bench.py --train
    --plumbing: everything else in this function is the code the GPU ranks run).
    With a `BucketAdamW` the tail behind the backward pass - clip and update - is `optimizer.step(clip_grad)` on csrc/grad_step.hip;
    with any other optimiser it is torch's, as before.  `grads_out`, a list: the reference's `vis.store_grads` - one `get_grads`
    record of the clipped gradients is appended per step (needs `buckets`).
    `amp`: False, True or "bf16" (bf16 autocast, no scaler needed), or "fp16" - the reference's numerics: fp16 autocast with a
    `scaler` (LossScaler; the loss is multiplied by its device scalar, the step's tail finds non-finite gradients, skips the update and
    moves the scale, see BucketAdamW.step).  As in the reference's loop the clip bounds the still-scaled norm; `clip_unscaled=True`
    is the textbook order (unscale, then clip - once, at the step).  `num_acc > 1`: the reference's gradient accumulation - the loss
    is divided by num_acc, a call with `step_now=False` adds its gradients to the running sum in the buckets and clips that sum IN
    PLACE (statistics, coefficient, hip.grad_scale), and the call with `step_now=True` steps; the call after it zeroes the buckets.
    The caller decides: step_now = (sample + 1) % num_acc == 0 or sample + 1 == len(loader).  The returned loss is the divided,
    unscaled one.
    `head`: "torch" (default) - the flows are summed over time and upsampled, and the loss is `flow_loss_supervised`'s torch
    composition; "hip" - the forward stops at the raw predictions (`forward_train_preds` / `forward_train_sew_preds`; an STTFlowNet's
    full-resolution flows count as factor-1 levels of one time step) and `flow_loss_hip` computes the loss and its gradient in two
    launches of csrc/flow_loss.hip.  Everything else - amp, the scaler, num_acc, n_valid over the ranks, the buckets, the tail - is the
    same code for both."""
    if head not in ("torch", "hip"):
        raise ValueError(f'train_step: head is "torch" or "hip", got {head!r}')
    if head == "hip" and forward_fn is not None:
        raise ValueError('train_step: head="hip" takes the raw decoder predictions of the HIP train-mode forward; a forward_fn returns '
                         'finished flow maps - use head="torch" with it')
    if isinstance(optimizer, BucketAdamW) and buckets is not optimizer.buckets:
        raise ValueError("train_step: a BucketAdamW steps on its GradientBuckets - pass them as buckets=")
    if grads_out is not None and buckets is None:
        raise ValueError("train_step: grads_out takes the statistics from the gradient buckets - pass buckets=")
    if amp not in (False, True, "bf16", "fp16"):
        raise ValueError(f'train_step: amp is False, True, "bf16" or "fp16", got {amp!r}')
    num_acc = int(num_acc)
    if num_acc < 1:
        raise ValueError(f"train_step: num_acc {num_acc}; it counts the micro-steps of one update (>= 1)")
    if (scaler is not None or num_acc > 1 or not step_now) and not isinstance(optimizer, BucketAdamW):
        raise NotImplementedError("train_step: a loss scaler and gradient accumulation live in the HIP tail of the step - use "
                                  "train.BucketAdamW over train.GradientBuckets as the optimiser (a scaler for the stock optimisers "
                                  "is not built)")
    if scaler is not None and not isinstance(scaler, LossScaler):
        raise TypeError("train_step: scaler is a train.LossScaler (load a torch.amp.GradScaler's state_dict() into one)")
    if (num_acc > 1 or not step_now) and dist is not None and world > 1:
        raise NotImplementedError("train_step: num_acc > 1 with world > 1 is not built - the bucket all-reduce would sum running sums; "
                                  "accumulate on one rank, or raise the per-rank batch instead")
    if amp == "fp16" and scaler is None:
        raise ValueError('train_step: amp="fp16" needs a loss scaler - pass scaler=train.LossScaler(), or use amp="bf16"')
    from .spikingjelly_compat import functional
    from .STSwinNet.STSwinNet import STTFlowNet
    from .STSwinNet_SNN.Spiking_STSwinNet import SpikingformerFlowNet
    ann = isinstance(model, STTFlowNet)             # the ANN family (train_flow_parallel_supervised.py): model(voxel, cnt)["flow"]
    if ann and amp:
        raise NotImplementedError("the ANN model trains in fp32 (configs/train_DSEC_supervised_STT_voxel.yml: use_amp False) - "
                                  "pass amp=False; fp16 for STTFlowNet is not built")
    model.train()
    if not ann:
        functional.reset_net(model)
    if buckets is not None:
        buckets.begin(dist, world, zero=not buckets.accumulating)
    else:
        optimizer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16 if amp == "fp16" else torch.bfloat16, enabled=bool(amp)):
        if forward_fn is not None:
            flows = forward_fn(model, chunk)
        elif ann:
            flows = model(chunk, None)["flow"]
            if head == "hip":
                flows = [f.unsqueeze(0) for f in flows]
        elif isinstance(model, SpikingformerFlowNet):
            flows = forward_train_sew_preds(model, chunk) if head == "hip" else forward_train_sew(model, chunk)
        else:
            flows = forward_train_preds(model, chunk) if head == "hip" else forward_train(model, chunk)
    n_valid = global_valid_count(mask, dist, world)
    # local mean over B_local of err_i / n_global, times 1 / world from the gradient average = the gathered-batch mean
    if head == "hip":
        loss = flow_loss_hip(flows, label, mask, flow_scaling, lambda_mod, n_valid=n_valid)
    else:
        loss = flow_loss_supervised([f.float() for f in flows], label, mask, flow_scaling, lambda_mod, n_valid=n_valid)
    if num_acc > 1:
        loss = loss / num_acc
    (loss if scaler is None else scaler.scale(loss)).backward()      # bucket all-reduces leave from the grad-ready hooks
    if buckets is not None:
        buckets.finish()
    if isinstance(optimizer, BucketAdamW):
        buckets.accumulating = not step_now
        if not step_now:                                             # the reference's clip of the running sum, in place; nothing is zeroed
            st = optimizer.stats
            clip_sum = clip_grad is not None and not clip_unscaled   # (the textbook order clips once, at the step)
            if clip_sum or grads_out is not None:
                st.compute()
            if clip_sum:
                st.clip(clip_grad, [p.grad is not None for p in st.params])
                st.scale_inplace()
        elif scaler is None:
            optimizer.step(clip_grad)
        else:
            optimizer.step(clip_grad, scaler=scaler, clip_unscaled=clip_unscaled)
        if grads_out is not None:
            grads_out.append(get_grads(model, buckets))
        return loss.detach()
    if clip_grad is not None:
        torch.nn.utils.clip_grad_norm_([p for p in model.parameters() if p.grad is not None], clip_grad)
    if grads_out is not None:                                        # (the gradients are clipped in place here: coef 1)
        grads_out.append(get_grads(model, buckets, coef=1.0))
    optimizer.step()
    return loss.detach()


# ---------------------------------------------------------------------------------------------- from a loader item to the step
def train_transform(config, finetune=False):
    """The loops' `transform_train` (train_flow_parallel_supervised_SNN.py:155-171): RandomCrop(loader.crop) - not when fine-tuning -
    then the two flips with loader.augment_prob[0] and [1]."""
    from .DSEC_dataloader.data_augmentation import Compose, RandomCrop, Random_horizontal_flip, Random_vertical_flip
    p = config["loader"]["augment_prob"]
    crop = [] if finetune else [RandomCrop(tuple(config["loader"]["crop"]))]
    return Compose(crop + [Random_horizontal_flip(p[0]), Random_vertical_flip(p[1])])


def _item_transform(config, transform):
    """`transform`, or for None the loops' `transform_valid`: CenterCrop(loader.crop) (nothing when the config has no crop)."""
    from .DSEC_dataloader.data_augmentation import CenterCrop, Compose
    if transform is not None:
        return transform
    crop = config["loader"].get("crop")
    return Compose([CenterCrop(tuple(crop))] if crop else [])


def prepare_train_item_torch(chunk, label, mask, config, transform, drop_u=None):
    """The loop's own sequence in torch (train_flow_parallel_supervised_SNN.py:241-308): the transforms on (chunk, label, mask), the
    polarity split / normalisation / threshold (harness.prepare_chunk) and, with metrics.mask_events, mask * event_mask.  What
    `prepare_train_item` is compared with, and what serves the configurations its kernel does not.  `drop_u`: the drop's uniform field
    in place of torch.rand_like.  Returns (x, label, mask (B, 1, h, w) fp32)."""
    from . import harness
    mask = mask.reshape(mask.shape[0], 1, *mask.shape[-2:]).float()
    chunk, label, mask = _item_transform(config, transform)((chunk, label, mask), drop_u)
    voxel = config["model"].get("encoding", "voxel") == "voxel"
    polarity = bool(config["loader"].get("polarity", True))
    if not voxel and polarity and chunk.dim() == 5:
        chunk = chunk.reshape(chunk.shape[0], -1, *chunk.shape[3:])
    x = harness.prepare_chunk(chunk, config["model"].get("norm_input"), config["data"].get("spike_th"), voxel and polarity)
    mask = mask.float()
    if config.get("metrics", {}).get("mask_events"):
        mask = mask * x.reshape(x.shape[0], -1, *x.shape[-2:]).sum(1, keepdim=True).bool()
    return x.contiguous(), label.contiguous(), mask.contiguous()


def prepare_train_item(chunk, label, mask, config, transform, step=0):
    """A loader item - signed voxel (B, bins, Hs, Ws), flow (B, 2, Hs, Ws), valid mask (B, Hs, Ws) or (B, 1, Hs, Ws), on the GPU - to
    `train_step`'s (x, label, mask): `transform.sample` draws the batch's crop origin, flips and drop rate as the reference's Compose
    does, and hip.augment_chunk (csrc/prepare_chunk.hip) applies them together with the loop's preparation in at most three launches,
    without asking the host; bit for bit `prepare_train_item_torch` given the same uniform field.  `transform` None: the loops'
    validation transform, CenterCrop(loader.crop).  Read from `config`: loader.crop (that case), model.norm_input, data.spike_th,
    metrics.mask_events, and for the drop's Philox stream loader.seed as the key and `step` as the offset (pass the iteration count: a
    step's field is then reproducible and no two steps share one).  `norm_input: std`, `loader.polarity: false` and the `cnt` encoding
    run the torch sequence."""
    norm = config["model"].get("norm_input")
    if norm not in (None, "minmax") or not config["loader"].get("polarity", True) or config["model"].get("encoding", "voxel") != "voxel":
        return prepare_train_item_torch(chunk, label, mask, config, transform)
    B = chunk.shape[0]
    p = _item_transform(config, transform).sample(chunk.shape)
    origins, flips, drop_q = p.per_sample(B)
    crop = None if tuple(p.crop) == tuple(chunk.shape[-2:]) else p.crop
    return hip.augment_chunk(chunk, label, mask, crop, origins, flips, drop_q=drop_q, seed=int(config["loader"].get("seed", 0)),
                             offset=int(step), norm_input=norm, spike_th=config["data"].get("spike_th"),
                             mask_events=bool(config.get("metrics", {}).get("mask_events")))


def train_step_from_item(model, optimizer, item, config, transform, step=0, **train_step_kwargs):
    """`train_step` on a loader item (chunk, label, mask): `prepare_train_item`, then the step unchanged.  Returns its loss."""
    chunk, label, mask = item
    x, label, mask = prepare_train_item(chunk, label, mask, config, transform, step=step)
    return train_step(model, optimizer, x, label, mask, **train_step_kwargs)


# ---------------------------------------------------------------------------------------------- from an MDR loader item to the step
def mdr_train_augmentor(config):
    """The MDR training set's augmentor (MDR_dataloader/MDR.py:65): DenseSparseAugmentor(loader.crop, loader.min_scale,
    loader.max_scale, do_flip=True)."""
    from .MDR_dataloader.loader_utils import DenseSparseAugmentor
    loader = config["loader"]
    return DenseSparseAugmentor(loader["crop"], min_scale=loader["min_scale"], max_scale=loader["max_scale"], do_flip=True)


def _mdr_volumes(sample, config):
    """(d_event_volume_old or None, d_event_volume_new, flow) of a loader dict: the pair the loop reads (train_mdr_supervised_SNN.py:
    209-214), the old volume only with data.num_chunks 2."""
    chunks = int(config["data"].get("num_chunks", 1))
    if chunks not in (1, 2):
        raise ValueError(f"data.num_chunks is 1 or 2, got {chunks}")
    return (sample["d_event_volume_old"] if chunks == 2 else None), sample["d_event_volume_new"], sample["flow"]


def _mdr_axis_torch(idx, n_src, f):
    """loader_utils._linear_axis on a device tensor of destination indices: (first tap, second tap, the second tap's weight fp32)."""
    c = ((idx.double() + 0.5) * (1.0 / float(f)) - 0.5).float()
    fl = c.floor()
    i, a = fl.long(), c - fl
    low, high = i < 0, i >= n_src - 1
    i = torch.where(low, torch.zeros_like(i), torch.where(high, torch.full_like(i, n_src - 1), i))
    return i, (i + 1).clamp(max=n_src - 1), torch.where(low | high, torch.zeros_like(a), a)


def prepare_mdr_item_torch(sample, config, augmentor, params=None):
    """`prepare_mdr_item` as a torch sequence on the tensors' device: per sample the index gathers of DenseSparseAugmentor under its
    record - the four taps combined in fp32 in cv2's order, one torch operation per product and sum; the flow scaled and the valid
    mask decided in fp64 - then the loop's cat, harness.prepare_chunk and mask * event_mask.  What the kernel is compared with, and what
    serves `norm_input: std`, `loader.polarity: false` (volumes (B, bins, 2, Hs, Ws)) and the `cnt` encoding.  Returns (x, label, mask
    (B, 1, h, w) fp32)."""
    from . import harness
    old, new, flow = _mdr_volumes(sample, config)
    B, (Hs, Ws), (h, w) = new.shape[0], new.shape[-2:], augmentor.crop_size
    params = augmentor.sample_batch(B, (Hs, Ws)) if params is None else params
    dev = new.device
    chunks, labels, masks = [], [], []
    for b, p in enumerate(params):
        vols = ([old[b]] if old is not None else []) + [new[b]]
        planes = torch.cat([v.reshape(-1, Hs, Ws).float() for v in vols] + [flow[b].float()])
        ys, xs = p.y0 + torch.arange(h, device=dev), p.x0 + torch.arange(w, device=dev)
        ys, xs = (p.size[0] - 1 - ys if p.vflip else ys), (p.size[1] - 1 - xs if p.hflip else xs)
        if p.resized:
            y0, y1, ay = _mdr_axis_torch(ys, Hs, p.scale_y)
            x0, x1, ax = _mdr_axis_torch(xs, Ws, p.scale_x)
            top, bot = planes[:, y0], planes[:, y1]
            top = top[:, :, x0] * (1 - ax) + top[:, :, x1] * ax
            bot = bot[:, :, x0] * (1 - ax) + bot[:, :, x1] * ax
            got = top * (1 - ay)[:, None] + bot * ay[:, None]
        else:
            got = planes[:, ys][:, :, xs]
        mul = [(p.scale_x if p.resized else 1.0) * (-1.0 if p.hflip else 1.0), (p.scale_y if p.resized else 1.0) * (-1.0 if p.vflip else 1.0)]
        f64 = got[-2:].double() * torch.tensor(mul, dtype=torch.float64, device=dev)[:, None, None]
        masks.append((~torch.isinf(f64[0]) & ~torch.isinf(f64[1]) & ((f64[0] * f64[0] + f64[1] * f64[1]).sqrt() > 0))[None].float())
        labels.append(f64.float())
        parts = torch.split(got[:-2], [v.numel() // (Hs * Ws) for v in vols])
        chunks.append(torch.cat([g.reshape(*v.shape[:-2], h, w) for g, v in zip(parts, vols)]))
    chunk, label, mask = torch.stack(chunks), torch.stack(labels), torch.stack(masks)
    voxel = config["model"].get("encoding", "voxel") == "voxel"
    polarity = bool(config["loader"].get("polarity", True))
    if not voxel and polarity and chunk.dim() == 5:
        chunk = chunk.reshape(chunk.shape[0], -1, *chunk.shape[3:])
    x = harness.prepare_chunk(chunk, config["model"].get("norm_input"), config["data"].get("spike_th"), voxel and polarity)
    if config.get("metrics", {}).get("mask_events"):
        mask = mask * x.reshape(x.shape[0], -1, *x.shape[-2:]).sum(1, keepdim=True).bool()
    return x.contiguous(), label.contiguous(), mask.contiguous()


def prepare_mdr_item(sample, config, augmentor, params=None):
    """An MDR loader item - the loader's dict with `d_event_volume_old`, `d_event_volume_new` (B, bins, Hs, Ws) and `flow`
    (B, 2, Hs, Ws), un-augmented, on the GPU - to `train_step`'s (x, label, mask): `augmentor.sample_batch` draws every item's scale,
    flips and crop origin as the reference's DenseSparseAugmentor does in Dataset.__getitem__ (`params`: records drawn already), and
    hip.augment_resize_chunk (csrc/prepare_chunk.hip) applies them together with the loop's cat, polarity split and preparation in at
    most three launches, without asking the host; bit for bit `prepare_mdr_item_torch` under the same records.  Read from `config`:
    data.num_chunks (1: the new volume alone), model.norm_input, data.spike_th, metrics.mask_events.  `norm_input: std`,
    `loader.polarity: false` and the `cnt` encoding run the torch sequence."""
    norm = config["model"].get("norm_input")
    if norm not in (None, "minmax") or not config["loader"].get("polarity", True) or config["model"].get("encoding", "voxel") != "voxel":
        return prepare_mdr_item_torch(sample, config, augmentor, params)
    old, new, flow = _mdr_volumes(sample, config)
    if params is None:
        params = augmentor.sample_batch(new.shape[0], tuple(new.shape[-2:]))
    return hip.augment_resize_chunk(old, new, flow, tuple(augmentor.crop_size), params, norm_input=norm,
                                    spike_th=config["data"].get("spike_th"),
                                    mask_events=bool(config.get("metrics", {}).get("mask_events")))


def train_step_from_mdr_item(model, optimizer, sample, config, augmentor, params=None, **train_step_kwargs):
    """`train_step` on an MDR loader item: `prepare_mdr_item`, then the step unchanged.  Returns its loss."""
    x, label, mask = prepare_mdr_item(sample, config, augmentor, params)
    return train_step(model, optimizer, x, label, mask, **train_step_kwargs)
