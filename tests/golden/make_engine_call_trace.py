#!/usr/bin/env python3
"""The launch schedule of sdformerflow_amd/engine.py as a call trace, taken WITHOUT a GPU: which C-ABI entry point every 3x3 spike
convolution, every decoder level and every prediction head goes to, on which weight representation, with how many images per call.

The routing code is plain Python on shapes, so it runs on `device="meta"` tensors: the engine object is made with `__new__`, packed
from a real (CPU) module tree, and the `hip` entry points it calls are replaced by recorders that return their output arguments.
What is traced per case: the patch embedding (its two strided convolutions and its res-blocks) and the whole U-Net tail (res-blocks,
decoders, prediction heads).

    python tests/golden/make_engine_call_trace.py          # rewrites tests/golden/engine_call_trace.json

tests/test_engine_routes_cpu.py re-runs `trace_all()` and compares it with that file record for record: a refactoring of the schedule
must reproduce it; a deliberate change of a route regenerates it and shows up as a diff of the JSON.
"""
import contextlib
import inspect
import json
import os
import sys
import types

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sdformerflow_amd import engine as E, hip                                                       # noqa: E402
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet_en4           # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "engine_call_trace.json")
CFG = os.path.join(ROOT, "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
META = torch.device("meta")
WIDTHS = (96, 192, 384, 768)                                      # en4: channels of the four encoder stages


# ------------------------------------------------------------------------------------------------ recorders
def _weights(Wp):
    """The weight representation a call multiplies by."""
    if Wp.dtype == torch.int16:
        return f"planes16x{Wp.shape[0]}"
    assert Wp.dtype == torch.int8, Wp.dtype
    return "digits_tiled" if getattr(Wp, "sdf_tiled", False) else "digits_rm"


def _epilogue(out, out_spike):
    return "both" if out is not None and out_spike is not None else ("spikes" if out_spike is not None else "fp32")


def _neuron_record(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, p, rowmap=None, rowlen=0, alpha=None, beta=None, Cch=0, inner=1, add=None,
                   add_st=0, add_period=0, v_last=None, rep=None):
    return {"T": T, "nb": nb, "ni": ni, "out": str(out.dtype).replace("torch.", ""), "kind": p.kind, "bn": alpha is not None,
            "rowmap": rowmap is not None, "rep": None if rep is None else rep[0]}


class Recorder:
    """Stand-ins for the `hip` launches and weight packers: every launch appends one record and returns its output argument."""

    def __init__(self):
        self.records = []

    def _add(self, fn, **kw):
        self.records.append(dict(fn=fn, **kw))

    # launches
    def spike_conv2d(self, x, Wp, imgs, H, W, Cin, OH, OW, KH, KW, stride, dy, dx, out=None, out_spike=None, alpha=None, beta=None,
                     resid=None, out_rowmap=None, sn=None, sn_T=0, pos=None):
        N = Wp.shape[1]
        assert x.numel() == imgs * H * W * Cin and Wp.shape[2] == KH * KW * Cin, "operand sizes do not match the call"
        for o in (out, out_spike):
            assert o is None or (o.numel() == imgs * OH * OW * N and o.is_contiguous()) or out_rowmap is not None
        assert resid is None or resid.numel() == imgs * OH * OW * N
        self._add("spike_conv2d", w=_weights(Wp), imgs=imgs, H=H, W=W, Cin=Cin, N=N, K=KH * KW * Cin, taps=[KH, KW], stride=stride,
                  x_img0=x.storage_offset() // (H * W * Cin), epi=_epilogue(out, out_spike), sn=None if sn is None else sn.kind,
                  T=sn_T if sn is not None else 0, bn=alpha is not None, resid=resid is not None, rowmap=out_rowmap is not None)
        return out if sn is None else out_spike

    def spike_conv2d_multi(self, x, classes, imgs, H, W, Cin, OH, OW, out, alpha=None, beta=None):
        assert x.numel() == imgs * H * W * Cin and all(c["rowmap"].numel() == imgs * H * W for c in classes)
        self._add("spike_conv2d_multi", w=_weights(classes[0]["Wp"]), classes=len(classes), imgs=imgs, H=H, W=W, Cin=Cin,
                  N=classes[0]["Wp"].shape[1], taps=[[c["KH"], c["KW"]] for c in classes], x_img0=x.storage_offset() // (H * W * Cin),
                  bn=alpha is not None)
        return out

    def spike_gemm(self, A, Wp, out, M, N, K, lda=None, ldo=None, bias=None, alpha=None, beta=None, resid=None, out_rowmap=None, zg=None):
        assert A.numel() == M * K and out.numel() == M * N and tuple(Wp.shape[1:]) == (N, K), "operand sizes do not match the call"
        self._add("spike_gemm", w=_weights(Wp), M=M, N=N, K=K, row0=A.storage_offset() // K, bias=bias is not None, bn=alpha is not None,
                  resid=resid is not None)
        return out

    def spike_deconv3x3s2(self, s, planes, imgs, T, H, W, Cin, Cout, alpha=None, beta=None, out=None, tiled_bn=False):
        assert s.numel() == imgs * H * W * Cin and out.numel() == imgs * 4 * H * W * Cout
        self._add("spike_deconv3x3s2", w=_weights(planes), imgs=imgs, T=T, H=H, W=W, Cin=Cin, Cout=Cout,
                  x_img0=s.storage_offset() // (H * W * Cin), bn=alpha is not None)
        return out

    def deconv_col2im(self, Y, imgs, H, W, Cout, alpha=None, beta=None, out=None):
        assert Y.numel() == imgs * H * W * 9 * Cout
        self._add("deconv_col2im", imgs=imgs, H=H, W=W, Cout=Cout, bn=alpha is not None)
        return out

    def neuron_fwd(self, x, out, *a, **k):
        self._add("neuron_fwd", **_neuron_record(x, out, *a, **k))
        return out

    def neuron_multi_fwd(self, calls):
        # (descriptors as argument tuples of neuron_fwd, or as (args, kwargs) pairs)
        pairs = [c if len(c) == 2 and isinstance(c[1], dict) else (c, {}) for c in calls]
        self._add("neuron_multi_fwd", descriptors=[_neuron_record(*a, **k) for a, k in pairs])

    def pred_head(self, z, wgt, bias, sn, H, W, want_pred=True, nxt=None, keep=False):
        B, D, h, w, Cin = z.shape
        self._add("pred_head", rows=B * D * h * w, Cin=Cin, kind=sn.kind, want_pred=bool(want_pred), feeds_next=nxt is not None,
                  flow=None if H is None else [H, W], keep=bool(keep),
                  next=None if nxt is None else {"ld": nxt[0].shape[4], "kind": nxt[1].kind, "z_off": nxt[2], "pred_off": nxt[3], "zero": list(nxt[4])})
        pred = torch.empty((B, D, h, w, 4), dtype=torch.float32, device=z.device) if want_pred else None
        flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=z.device) if H is not None else None
        return pred, flow, (torch.empty((B, D, h, w, Cin), dtype=torch.uint8, device=z.device) if keep else None)

    def head_conv_sn(self, x, w, B, T, H, W, p, alpha=None, beta=None, voxel_bins=None):
        self._add("head_conv_sn", B=B, T=T, H=H, W=W, Cin=w.shape[1], Cout=w.shape[0], kind=p.kind, bn=alpha is not None)
        return torch.empty((B, T, H, W, w.shape[0]), dtype=torch.uint8, device=x.device)

    def pointwise_conv_f32(self, x, w, stride, bias=None):
        imgs, H, W, Cin = x.shape
        self._add("pointwise_conv_f32", imgs=imgs, H=H, W=W, Cin=Cin, N=w.shape[0], stride=stride)
        return torch.empty((imgs, (H - 1) // stride + 1, (W - 1) // stride + 1, w.shape[0]), dtype=torch.float32, device=x.device)

    # weight packers: meta tensors that carry the attributes the launches (and the routing) look at
    @staticmethod
    def split_weight(W, nsplit=3):
        planes = torch.empty((nsplit,) + tuple(W.shape), dtype=torch.int16, device=META)
        if nsplit == 2:
            planes.sdf_acc_scale = 1.0
        return planes

    @staticmethod
    def split_weight_i8x3(W):
        planes = torch.empty((3,) + tuple(W.shape), dtype=torch.int8, device=META)
        planes.sdf_col_scale = torch.empty((W.shape[0],), dtype=torch.float32, device=META)
        return planes

    @staticmethod
    def tile_weight_i8x3(planes):
        tiled = torch.empty_like(planes)
        tiled.sdf_col_scale, tiled.sdf_tiled = planes.sdf_col_scale, True
        return tiled

    @staticmethod
    def pack_deconv2x2_weight(w, cin_pad):
        return Recorder.split_weight_i8x3(torch.empty((4 * w.shape[1], 4 * cin_pad), device=META))


PATCHED = ("spike_conv2d", "spike_conv2d_multi", "spike_gemm", "spike_deconv3x3s2", "deconv_col2im", "neuron_fwd", "neuron_multi_fwd",
           "pred_head", "head_conv_sn", "pointwise_conv_f32", "split_weight", "split_weight_i8x3", "tile_weight_i8x3", "pack_deconv2x2_weight")


@contextlib.contextmanager
def recording(rec):
    """`hip`'s launches and packers replaced by `rec`'s for the block."""
    saved = {n: getattr(hip, n) for n in PATCHED}
    try:
        for n in PATCHED:
            setattr(hip, n, getattr(rec, n))
        yield rec
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)


# ------------------------------------------------------------------------------------------------ engine on meta tensors
_MODELS = {}


def _model(kind, T):
    if (kind, T) not in _MODELS:
        cfg = yaml.safe_load(open(CFG))
        cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind, num_steps=T)
        cfg["model"]["num_bins"] = T
        cfg["swin_transformer"]["input_size"] = [288, 384]          # (sizes the window tables only: no traced layer reads it)
        _MODELS[(kind, T)] = MS_SpikingformerFlowNet_en4(cfg["model"].copy(), cfg["swin_transformer"].copy()).eval()
    return _MODELS[(kind, T)]


def make_engine(kind, T, nsplit):
    """MSFlowEngine of the en4 model with every packed tensor on the meta device (call under `recording`): what __init__ sets for
    the patch embedding, and the engine's own `_init_stages` (without swin stages) for res-blocks, decoders and prediction heads."""
    model = _model(kind, T)
    unet = model.sttmultires_unet
    pe = unet.encoders.swin3d.patch_embed
    eng = E.MSFlowEngine.__new__(E.MSFlowEngine)
    eng.device, eng.nsplit = META, nsplit
    eng.num_bins, eng.num_steps = pe.num_bins, pe.num_steps
    eng.head_w = pe.head.conv[0].weight.detach().to(META)
    eng.head_w_oihw = pe.head.conv[0].weight.detach().float().to(META)
    eng.head_bn, eng.head_sn = E.bn_affine(pe.head.norm_layer.norm_layer, META), E._np(pe.head.sn, META)
    eng.conv_w, eng.conv_bn = E._conv_planes(pe.conv.conv[0].weight, nsplit), E.bn_affine(pe.conv.norm_layer.norm_layer, META)
    eng.conv_w.digits = E._conv_digits(pe.conv.conv[0].weight, nsplit)
    U = "sttmultires_unet."
    eng.pe_name = U + "encoders.swin3d.patch_embed."
    eng.pe_res = [E._ResBlock(rb, META, nsplit, eng.pe_name + f"residual_encoding.resblocks.{i}.") for i, rb in enumerate(pe.residual_encoding.resblocks)]
    eng.proj_res_w = pe.proj.conv_res.weight.detach().to(META)
    eng.proj_res_w2 = pe.proj.conv_res.weight.detach().float().reshape(pe.proj.conv_res.weight.shape[0], -1).to(META)
    eng.proj_res_b = None if pe.proj.conv_res.bias is None else pe.proj.conv_res.bias.detach().float().to(META)
    eng.proj_w = E._conv_planes(pe.proj.conv.weight, nsplit)
    eng.proj_w.digits = E._conv_digits(pe.proj.conv.weight, nsplit)
    eng.proj_bn, eng.proj_sn = E.bn_affine(pe.proj.norm_layer, META), E._np(pe.proj.sn, META)
    eng._maps, eng._deconv, eng.tape, eng.scores, eng.replicas = {}, {}, None, None, False
    eng._init_stages(model, unet, types.SimpleNamespace(layers=[]), META, nsplit, U)
    return eng


def pyramid(B, T, H, W):
    """Encoder features of a (H, W) input: stage i at 1/4 of the input halved i times (odd sizes round up), WIDTHS[i] channels."""
    h, w, feats = H // 4, W // 4, []
    for c in WIDTHS:
        feats.append(torch.empty((B, T, h, w, c), dtype=torch.float32, device=META))
        h, w = (h + 1) // 2, (w + 1) // 2
    return feats


# name, neuron, T, (H, W), batch, replicas, weight planes, tape, switches
def cases():
    out = [("c1_lif", "lif", 10, (288, 384), 1, False, 2, False, {}),
           ("c1_lif_tape", "lif", 10, (288, 384), 1, False, 2, True, {})]
    out += [(f"c1_lif_R{R}", "lif", 10, (288, 384), R, True, 2, False, {}) for R in (2, 4, 7, 10, 40)]
    out += [("c1_psn", "psn", 10, (288, 384), 1, False, 2, False, {}), ("c1_psn_R10", "psn", 10, (288, 384), 10, True, 2, False, {})]
    out += [("c4_lif_B4", "lif", 20, (480, 640), 4, False, 2, False, {}), ("c4_lif_R2", "lif", 20, (480, 640), 2, True, 2, False, {})]
    out += [(f"small_lif_R{R}", "lif", 10, (144, 192), R, True, 2, False, {}) for R in (3, 4)]
    out += [("planes3_lif", "lif", 10, (288, 384), 1, False, 3, False, {}), ("planes3_lif_R3", "lif", 10, (288, 384), 3, True, 3, False, {})]
    out += [("mdr_psn_T5", "psn", 5, (256, 256), 1, False, 2, False, {})]
    out += [("odd_lif", "lif", 10, (300, 400), 1, False, 2, False, {})]         # 75 x 100 -> 38 x 50 -> 19 x 25 -> 10 x 13: the concatenation path
    out += [(f"c1_lif_{k}_0", "lif", 10, (288, 384), 1, False, 2, False, {k: "0"})
            for k in ("SDF_SMALLM", "SDF_CONV_WRES", "SDF_RES_GEMM", "SDF_DECONV_GEMM")]
    return out


def trace_case(kind, T, size, B, replicas, nsplit, tape, switches, engines=None):
    """{"patch_embed": [records], "unet_tail": [records]} of one case."""
    H, W = size
    out = {}
    with hip.scoped_switches(**switches), recording(Recorder()) as rec:
        key = (kind, T, nsplit)
        eng = engines.get(key) if engines is not None else None
        if eng is None:
            eng = make_engine(kind, T, nsplit)
            if engines is not None:
                engines[key] = eng
        eng.replicas, eng.tape = replicas, ([] if tape else None)
        try:
            for part, call in (("patch_embed", lambda: eng.patch_embed(torch.empty((B, T, 2, H, W), dtype=torch.float32, device=META))),
                               ("unet_tail", lambda: eng.unet_tail(pyramid(B, T, H, W), out_size=(H, W)))):
                rec.records = []
                call()
                out[part] = rec.records
        finally:
            eng.replicas, eng.tape = False, None
    return out


def trace_all():
    engines = {}
    return {c[0]: trace_case(*c[1:], engines=engines) for c in cases()}


def _text(v):
    if isinstance(v, dict):
        return "{" + " ".join(k if x is True else f"{k}={_text(x)}" for k, x in sorted(v.items()) if k != "fn" and x not in (False, None)) + "}"
    return "[" + ",".join(_text(x) for x in v) + "]" if isinstance(v, (list, tuple)) else str(v)


def lines(records):
    """One line per record: the entry point, then `key=value` of everything that is set (False / None / 0 are left out, True is the bare key).  Calls in a
    row that differ only in where their chunk starts (`x_img0`, `row0`) share a line that lists the starts as `at=[...]`."""
    out = []
    for r in records:
        start = r.get("x_img0", r.get("row0"))
        body = {k: v for k, v in r.items() if k not in ("x_img0", "row0")}
        if out and out[-1][0] == body and start is not None:
            out[-1][1].append(start)
        else:
            out.append((body, [start]))
    return [b["fn"] + " " + _text(dict(b, at=at if len(at) > 1 else at[0]))[1:-1] for b, at in out]


def dumps(trace):
    """{case: {part: [line per record]}}, one record per line (a route change then reads as a line diff); a part that equals the same
    part of an earlier case names that case instead."""
    out, seen = ["{"], {}
    for ci, (name, parts) in enumerate(trace.items()):
        out.append(f' {json.dumps(name)}: {{')
        for pi, (part, records) in enumerate(parts.items()):
            ls, end = lines(records), "," if pi + 1 < len(parts) else ""
            first = seen.setdefault((part, tuple(ls)), name)
            if first != name:
                out.append(f'  {json.dumps(part)}: {json.dumps("= " + first)}{end}')
            else:
                out += [f'  {json.dumps(part)}: ['] + [f'   {json.dumps(l)}{"," if i + 1 < len(ls) else ""}' for i, l in enumerate(ls)] + ["  ]" + end]
        out.append(" }" + ("," if ci + 1 < len(trace) else ""))
    return "\n".join(out + ["}"]) + "\n"


if __name__ == "__main__":
    assert inspect.signature(hip._neuron_desc).parameters.keys() == inspect.signature(_neuron_record).parameters.keys()
    text = dumps(trace_all())
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {len(cases())} cases, {text.count(chr(10))} lines, {len(text)} bytes")
