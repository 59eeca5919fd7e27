"""Training with GLIF and SLTT-LIF neurons (`neuron_type: glif`, `SLTTlif`) on the GPU: the GLIF forward / BPTT kernels with the
gradient of the derived gate table (csrc/glif.hip) and the LIF BPTT kernel with the membrane detached between steps (csrc/neuron_bwd.hip
sdf_sltt_bwd) against fixtures made by the REAL reference's autograd (tests/golden/make_golden_glif_train.py); a train-mode block,
a train step of each, and the argument refusals of the new entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import sdformer_oracle as O
from sdformerflow_amd import hip, train
from sdformerflow_amd.STSwinNet_SNN import Spiking_swin_transformer3D as SW
from sdformerflow_amd.STSwinNet_SNN.Spiking_modules import Spiking_neuron
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet
from sdformerflow_amd.STSwinNet_SNN.Spiking_submodules import GatedLIFNode, SLTTLIFNode
from sdformerflow_amd.synthetic import synth_label, synth_state_dict, synth_uniform as rnd, synth_voxel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GG = np.load(os.path.join(HERE, "golden", "glif_grads.npz"))
SG = np.load(os.path.join(HERE, "golden", "sltt_grads.npz"))
GB = np.load(os.path.join(HERE, "golden", "glif_train_block.npz"))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
SHAPES = {"N256": (256,), "N105": (3, 7, 5), "N3076": (3076,)}
GATES = ("alpha", "beta", "gamma", "tau", "v_threshold", "linear_decay", "v_subreset", "conduct")
RESETS = {"soft": None, "hard": 0.0, "hard005": 0.05}
_CASES = {}


def case(T, tag):
    """(x, dL/ds) of the generator from its seeds, the tie and the hard-driven column blocks overwritten as it does; made once."""
    if (T, tag) not in _CASES:
        shape, si = SHAPES[tag], list(SHAPES).index(tag)
        N = int(np.prod(shape))
        blk = 64 if N >= 256 else 8
        x0 = (3.0 * rnd((T,) + shape, 1000 + 10 * T + si, -0.3, 0.6)).reshape(T, N)
        assert int(GG[f"T{T}_ties"]) > 0                             # u - th == 0 exactly at t = 0 in these columns
        x0[0, :blk] = float(GG[f"T{T}_tie_x"])
        x0[:, blk:2 * blk] = 2.5
        _CASES[T, tag] = (x0.reshape((T,) + shape), rnd((T,) + shape, 1100 + 10 * T + si, -1.0, 2.0))
    return _CASES[T, tag]


def logits(T):
    return {k: torch.from_numpy(GG[f"T{T}/spiking_neuron.{k}"]) for k in GATES}


def table_of(*lg):
    """The derived table from the gate logits (GATES order), the products in the reference's order."""
    s = dict(zip(GATES, (torch.sigmoid(v) for v in lg)))
    head = torch.stack([1 - s["alpha"] * (1 - s["tau"]), (1 - s["alpha"]) * s["linear_decay"], s["gamma"],
                        (1 - s["gamma"]) * s["v_subreset"], s["v_threshold"]])
    return torch.cat([head, 1 - s["beta"] * (1 - s["conduct"])])


@pytest.mark.parametrize("T", [2, 4, 10])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_glif_forward_is_bit_equal_to_the_reference(T, tag):
    """The fixture's CPU-computed table: spikes bit-equal, fp32 and u8.  The module builds the table with device sigmoids, which may
    flip decisions at the threshold: at most 1e-3 of them (the condition of test_hip_kernels' glif case)."""
    x0, _ = case(T, tag)
    want = torch.from_numpy(GG[f"T{T}_{tag}_s"])
    sd = {"spiking_neuron." + k: v for k, v in logits(T).items()}
    assert torch.equal(O.glif_multistep(x0, sd, "spiking_neuron.").to(torch.uint8), want)       # the oracle's restatement: 0 differ
    tab = torch.from_numpy(GG[f"T{T}_tab"])
    assert torch.equal(table_of(*logits(T).values()), tab)
    x = x0.to(DEV)
    s32, s8 = hip.glif_fwd(x, tab.to(DEV)), hip.glif_fwd(x, tab.to(DEV), torch.uint8)
    assert s32.dtype == torch.float32 and s8.dtype == torch.uint8 and s32.shape == x.shape
    assert torch.equal(s32.to(torch.uint8).cpu(), want) and torch.equal(s8.cpu(), want)
    m = Spiking_neuron(num_steps=T, neuron_type="glif").to(DEV).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        got = m(x)
    assert (got.to(torch.uint8).cpu() != want).float().mean().item() <= 1e-3


@pytest.mark.parametrize("T", [2, 4, 10])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_glif_backward_matches_reference_autograd(T, tag):
    """dL/dx within 1e-6 of the fixture's largest |dL/dx|; every logit's gradient - grad_tab chained through the table expression -
    within 1e-5 of the sum of the absolute values of the terms it sums (the fixture's `gtab_abs`, carried through |d tab / d logit|):
    the bounds test_plif_train_gpu.py holds dL/dx and dL/dw to.  grad_tab itself is also held to the generator's fp64 evaluation of
    the same recurrence at the same bound.  Two calls: bit-equal."""
    x0, g0 = case(T, tag)
    key = f"T{T}_{tag}"
    tab = torch.from_numpy(GG[f"T{T}_tab"])
    x, g = x0.to(DEV), g0.to(DEV)
    gx, gtab = hip.glif_bwd(x, tab.to(DEV), g, 2.0)
    gx_ref = torch.from_numpy(GG[f"{key}_gx"]).reshape(x0.shape)
    dev_x = (gx.cpu() - gx_ref).abs().max().item()
    print(f"{key}: max |dgx| {dev_x:.3e} (bound {1e-6 * gx_ref.abs().max().item():.3e})")
    assert dev_x <= 1e-6 * gx_ref.abs().max().item()
    gt64, gabs = torch.from_numpy(GG[f"{key}_gtab64"]), torch.from_numpy(GG[f"{key}_gtab_abs"])
    dev_t = (gtab.cpu().double() - gt64).abs()
    print(f"{key}: max |dgtab| / sum|terms| {float((dev_t / gabs.clamp_min(1e-30)).max()):.3e}")
    assert bool((dev_t <= 1e-5 * gabs).all()), (dev_t, gabs)
    lg = tuple(v.double() for v in logits(T).values())
    jac = torch.autograd.functional.jacobian(table_of, lg)           # per logit: (5 + T, *logit shape)
    for k, J in zip(GATES, jac):
        J = J.reshape(5 + T, -1)
        got = (gtab.cpu().double()[:, None] * J).sum(0)
        bound = 1e-5 * (gabs[:, None] * J.abs()).sum(0)
        ref = torch.from_numpy(GG[f"{key}_g/{k}"]).double().reshape(-1)
        assert bool(((got - ref).abs() <= bound).all()), (k, got, ref, bound)
    again = hip.glif_bwd(x, tab.to(DEV), g, 2.0)
    assert torch.equal(again[0], gx) and torch.equal(again[1], gtab)


@pytest.mark.parametrize("T", [2, 4, 10])
def test_glif_padded_columns_add_nothing_to_the_table_gradient(T):
    """N = 105 (the wrapper pads it to 108) against the same data embedded in N = 108 and N = 112 with zero x and zero dL/ds: a padded
    column has dL/du_t = 0 at every step, so grad_tab is bit-equal."""
    x0, g0 = case(T, "N105")
    tab = torch.from_numpy(GG[f"T{T}_tab"]).to(DEV)
    gx, gtab = hip.glif_bwd(x0.to(DEV), tab, g0.to(DEV), 2.0)
    assert gx.shape == x0.shape
    for n in (108, 112):
        xe, ge = torch.zeros(T, n), torch.zeros(T, n)
        xe[:, :105], ge[:, :105] = x0.reshape(T, 105), g0.reshape(T, 105)
        gxe, gtabe = hip.glif_bwd(xe.to(DEV), tab, ge.to(DEV), 2.0)
        assert torch.equal(gtabe, gtab), n
        assert torch.equal(gxe[:, :105].reshape(x0.shape), gx) and not gxe[:, 105:].any()


@pytest.mark.parametrize("T", [2, 4, 10])
@pytest.mark.parametrize("tag", list(RESETS))
def test_sltt_online_gradient_matches_reference_autograd(T, tag):
    v_th, v_reset = float(SG["v_th"]), RESETS[tag]
    x0 = rnd((T, 256), 1200 + T, -0.3, 0.6)
    x0[:, :64] = 0.1
    assert int(SG[f"{tag}_T{T}_ties"]) > 0
    x0[0, 64:128] = float(SG[f"{tag}_T{T}_tie_x"])
    g = rnd((T, 256), 1300 + T, -1.0, 2.0).to(DEV)
    got = {}
    for detach in (True, False):
        key = f"{tag}_{'detach' if detach else 'nodetach'}_T{T}"
        node = SLTTLIFNode(tau=2.0, v_threshold=v_th, v_reset=v_reset, surrogate_function=None, detach_reset=detach).train()
        x = x0.to(DEV).requires_grad_(True)
        s = node(x)
        s.backward(g)
        assert torch.equal(s.detach().to(torch.uint8).cpu(), torch.from_numpy(SG[f"{key}_s"]))
        gx_ref = torch.from_numpy(SG[f"{key}_gx"])
        dev = (x.grad.cpu() - gx_ref).abs().max().item()
        print(f"sltt {key}: max |dgx| {dev:.3e} (bound {1e-6 * gx_ref.abs().max().item():.3e})")
        assert dev <= 1e-6 * gx_ref.abs().max().item()
        got[detach] = x.grad
    assert torch.equal(got[True], got[False])                       # the reset only feeds the detached membrane


def kw(kind, T):
    return {"num_steps": T, "v_reset": None, "v_th": 0.1, "neuron_type": kind, "surrogate_fun": "surrogate.ATan()", "tau": 2.0,
            "detach_reset": True, "spike_norm": "BN"}


def rate(got, ref):
    got, ref = got.detach().float().cpu(), torch.as_tensor(ref).float()
    assert got.shape == ref.shape
    scale = ref.abs().mean().item() + 1e-12
    return ((got - ref).abs() > 1e-3 * scale).float().mean().item()


def picked(t, key):
    """The elements of t the fixture kept under `key` (all of them, or those at `key@idx`), flattened."""
    t = t.detach().reshape(-1)
    return t[torch.from_numpy(GB[key + "@idx"]).long().to(t.device)] if key + "@idx" in GB.files else t


def test_glif_train_mode_block_matches_reference_autograd():
    """The tolerances of test_plif_train_gpu's block test: mismatch rates over the sampled elements, and every gate logit's gradient
    within 1e-3 of its reference value."""
    B, H, W, *shift = (int(v) for v in GB["cfg"])
    blk = SW.MS_Spiking_SwinTransformerBlock3D(96, (H, W), 3, window_size=(2, 9, 9), shift_size=tuple(shift), norm_layer="BN",
                                               **kw("glif", 4))
    blk.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}), strict=True)
    with torch.no_grad():
        for k in GB.files:
            if k.startswith("w/"):
                blk.get_parameter(k[2:]).copy_(torch.from_numpy(GB[k]))
    blk = blk.to(DEV).train()
    x = rnd((B, 4, H, W, 96), 17, -0.5, 1.0).to(DEV).requires_grad_(True)
    g = rnd((B, 4, H, W, 96), 18, -1.0, 2.0).to(DEV)
    y = train.ms_block(x, blk, training=True)
    y.backward(g)
    report = {"y": rate(picked(y, "y"), GB["y"]), "gx": rate(picked(x.grad, "gx"), GB["gx"])}
    params = dict(blk.named_parameters())
    nodes = set()
    for k in GB.files:
        if not k.startswith("g/") or k.endswith("@idx"):
            continue
        name = k[2:]
        if ".spiking_neuron." in name:
            got, ref = params[name].grad.detach().cpu().reshape(-1), torch.from_numpy(GB[k]).reshape(-1)
            print(f"{name}: {got.tolist()} ref {ref.tolist()}")
            assert bool(((got - ref).abs() <= 1e-3 * ref.abs()).all()), (name, got, ref)
            nodes.add(name.rsplit(".spiking_neuron.", 1)[0])
        elif name.endswith("proj.bias"):
            assert params[name].grad.abs().max().item() < 1e-3 * float(np.abs(GB["g/attn.proj.weight"]).mean())
        else:
            report[name] = rate(picked(params[name].grad, k), GB[k])
    for k in GB.files:
        if k.startswith("r/"):
            report["running:" + k[2:]] = rate(picked(dict(blk.named_buffers())[k[2:]], k), GB[k])
    assert len(nodes) == 6, nodes                                     # sn_q, sn_k, sn2_q (the gate), proj_sn, mlp.sn1, mlp.sn2
    worst = max(report.values())
    print(f"glif train block: mismatch rates y {report['y']:.2e} gx {report['gx']:.2e} worst {worst:.2e}")
    assert report["y"] <= 2e-3 and report["gx"] <= 5e-3 and worst <= 1e-2, report


def small_model(kind):
    """The 3-encoder model test_plif_train_gpu builds; GLIF gate logits are drawn as the fixtures draw them."""
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"].update(input_size=[144, 144], swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])
    model = MS_SpikingformerFlowNet(cfg["model"].copy(), cfg["swin_transformer"].copy())
    model.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    with torch.no_grad():
        for i, (n, p) in enumerate(model.named_parameters()):
            if isinstance(model.get_submodule(n.rsplit(".", 1)[0]), GatedLIFNode):
                p.copy_(rnd(tuple(p.shape), 5000 + i, -1.0, 2.0))
    model = model.to(DEV).train()
    for m in model.modules():
        if hasattr(m, "drop_path_rate"):
            m.drop_path_rate = 0.0
    from sdformerflow_amd import harness
    chunk = harness.prepare_chunk(synth_voxel(2, 10, 144, 144, seed=1234 + 4)).to(DEV)
    label, mask = synth_label(2, 144, 144)
    return model, chunk, label.to(DEV), mask.to(DEV)


@pytest.mark.parametrize("kind", ["glif", "SLTTlif"])
def test_train_step_runs_and_moves_the_parameters(kind):
    model, chunk, label, mask = small_model(kind)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    loss = train.train_step(model, opt, chunk, label, mask, buckets=train.GradientBuckets(model.parameters()))
    assert torch.isfinite(loss).all()
    moved = [n for n, p in model.named_parameters() if p.grad is not None and not torch.equal(p.detach(), before[n])]
    assert len(moved) > 100
    if kind == "glif":
        gates = [(n, p) for n, p in model.named_parameters() if isinstance(model.get_submodule(n.rsplit(".", 1)[0]), GatedLIFNode)]
        unused = [n for n, p in gates if p.grad is None]
        assert all(".attn_sn." in n for n in unused), unused          # the score neuron runs under log=True only
        used = [(n, p) for n, p in gates if p.grad is not None]
        assert len(used) > 50 * 8
        for n, p in used:
            assert torch.isfinite(p.grad).all() and bool((p.grad != 0).all()), (n, p.grad)
            assert not torch.equal(p.detach(), before[n]), n


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    L = hip.lib()
    p, E_SHAPE = C.c_void_p(0x10000), -2

    def gfwd(T=10, N=4096):
        return L.sdf_glif_fwd(p, p, p, T, N, 0, None)

    def gbwd(T=10, N=4096, wsb=1 << 20, surrogate=0):
        return L.sdf_glif_bwd(p, p, p, p, p, p, wsb, T, N, surrogate, 2.0, None)

    def sbwd(T=10, N=4096, surrogate=0):
        return L.sdf_sltt_bwd(p, p, p, T, N, 2.0, 0.1, 1, 0.0, surrogate, 2.0, None)

    assert gfwd(T=3) == E_SHAPE and gbwd(T=3) == E_SHAPE and sbwd(T=3) == E_SHAPE
    assert gfwd(T=8) == E_SHAPE and gfwd(N=4094) == E_SHAPE and gbwd(N=4094) == E_SHAPE and sbwd(N=4094) == E_SHAPE
    assert gbwd(surrogate=1) == E_SHAPE and sbwd(surrogate=1) == E_SHAPE
    need = L.sdf_glif_bwd_workspace_bytes(10, 4096)
    assert need == 4 * 15 * 4 and gbwd(wsb=need - 1) == E_SHAPE
    assert L.sdf_glif_bwd_workspace_bytes(3, 4096) == 0
    assert L.sdf_glif_fwd(None, p, p, 10, 4096, 0, None) == -1 and L.sdf_glif_fwd(p, p, p, 10, 4096, 7, None) == -3
