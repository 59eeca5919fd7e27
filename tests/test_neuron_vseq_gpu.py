"""sdf_neuron_vseq_fwd (csrc/neuron.hip neuron_vseq_kernel, hip.neuron_fwd(..., v_seq=)): the general neuron launch that also writes
the membrane after reset of every step.

Per case: the spikes are bit-equal to sdf_neuron_fwd's on the same descriptor and to the oracle's; v_seq is bit-equal to the prefix
reference `oracle.neuron_ref(x[:t+1], ..., return_aux=True)[1]`, t = 0 .. T-1 (tests/test_membrane_cpu.py ties that form to
spikingjelly's `store_v_seq`); v_last is v_seq's last step.  N = 1028 neurons per step: one full workgroup of 256 quads and a partial
one.  `out` and `v_seq` lie inside larger buffers of a sentinel value and are compared WHOLE - the guard regions in front and behind
and the gaps that strides larger than the problem leave must come back untouched."""
import pytest
import torch

from oracle.neuron_ref import neuron_ref
from sdformerflow_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 1028
GUARD = 64                    # elements in front of and behind the addressed region
S_U8, S_F32 = 7, -123.0       # sentinels no spike (0 / 1) and no membrane of these inputs (|v| < 1) can equal
NEURONS = {"lif_soft": ("lif", 2.0, None), "lif_hard": ("lif", 3.0, -0.05), "if": ("if", 2.0, None)}
V_TH = 0.1


def rand(shape, seed, lo=-0.3, hi=0.6):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def prefix_reference(x, kind, tau, v_reset, **kw):
    """x (T, n) effective inputs -> (spikes (T, n), v_seq (T, n)): the membrane after step t is the final state of a run on x[:t+1]."""
    T = x.shape[0]
    add = kw.pop("add", None)
    runs = [neuron_ref(x[:t + 1], kind, tau, V_TH, v_reset, return_aux=True, add=None if add is None else add[:t + 1], **kw) for t in range(T)]
    return runs[-1][0], torch.stack([v for _, v in runs])


def check(T, neuron, out_dtype, x_dev, x_eff, offsets, span, launch_kw, ref_kw=None, problems=1):
    """Launch with and without v_seq on the same descriptor; `offsets` (T, problems * n) = where element (t, i) of the effective problem
    lies in out / v_seq (elements), `span` = the addressed region's length."""
    kind, tau, v_reset = NEURONS[neuron]
    p = hip.NeuronParams(kind, tau, V_TH, v_reset)
    sent = S_U8 if out_dtype == torch.uint8 else S_F32
    bufs = {k: torch.full((GUARD + span + GUARD,), sent, dtype=out_dtype, device=DEV) for k in ("plain", "vseq")}
    vbuf = torch.full((GUARD + span + GUARD,), S_F32, dtype=torch.float32, device=DEV)
    n_all = x_eff.shape[1]
    v_last = {k: torch.full((n_all,), S_F32, dtype=torch.float32, device=DEV) for k in bufs}
    args = launch_kw.pop("args")
    hip.neuron_fwd(x_dev, bufs["plain"][GUARD:], T, *args, p, v_last=v_last["plain"], **launch_kw)
    with hip.launch_log() as log:
        hip.neuron_fwd(x_dev, bufs["vseq"][GUARD:], T, *args, p, v_last=v_last["vseq"], v_seq=vbuf[GUARD:], **launch_kw)
    torch.cuda.synchronize()
    assert len(log.rows) == 1 and "neuron_vseq_kernel" in log.rows[0][0], log.rows
    assert log.rows[0][1] == -(-(n_all // 4) // 256) and log.rows[0][2] == 256
    assert torch.equal(bufs["plain"], bufs["vseq"]), "spikes differ from sdf_neuron_fwd's"
    assert torch.equal(v_last["plain"], v_last["vseq"])
    n = n_all // problems
    s_ref, v_ref = [], []
    for k in range(problems):                                   # (the oracle's channel / period index runs over ONE problem)
        s, v = prefix_reference(x_eff[:, k * n:(k + 1) * n].contiguous(), kind, tau, v_reset, **dict(ref_kw or {}))
        s_ref.append(s)
        v_ref.append(v)
    s_ref, v_ref = torch.cat(s_ref, 1), torch.cat(v_ref, 1)
    want_s = torch.full((GUARD + span + GUARD,), sent, dtype=out_dtype)
    want_v = torch.full((GUARD + span + GUARD,), S_F32, dtype=torch.float32)
    want_s[GUARD + offsets.reshape(-1)] = s_ref.reshape(-1).to(out_dtype)
    want_v[GUARD + offsets.reshape(-1)] = v_ref.reshape(-1)
    assert torch.equal(bufs["vseq"].cpu(), want_s), "spikes differ from the oracle's (or a guard byte was written)"
    got_v = vbuf.cpu()
    assert torch.equal(got_v.view(torch.int32), want_v.view(torch.int32)), \
        f"v_seq is not the prefix reference bit for bit (or a guard was written): max |dv| {(got_v - want_v).abs().max().item():.3e}"
    assert torch.equal(v_last["vseq"].cpu().view(torch.int32), v_ref[-1].view(torch.int32))
    assert 0 < int(s_ref.sum()) < s_ref.numel()                 # (the inputs make the neurons fire, and not always)


def dense(T, seed=0):
    x = rand((T, N), seed)
    off = torch.arange(T).view(T, 1) * N + torch.arange(N).view(1, N)
    return x, off, dict(args=(1, N, 0, N, 0, N))


@pytest.mark.parametrize("out_dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("neuron", list(NEURONS))
@pytest.mark.parametrize("T", [2, 4, 5, 10, 20, 3])
def test_dense_every_T_neuron_and_spike_dtype(T, neuron, out_dtype):
    """The compiled T values and a runtime T of 3; LIF soft reset (tau 2: the exact reciprocal), LIF hard reset to a non-zero v_reset with
    tau 3 (the division), IF; u8 and fp32 spikes."""
    x, off, kw = dense(T, seed=T)
    check(T, neuron, out_dtype, x.to(DEV), x, off, T * N, kw)


@pytest.mark.parametrize("T", [10, 3])
@pytest.mark.parametrize("inner,Cch", [(1, 4), (8, 3)])
def test_bn_affine(T, inner, Cch):
    x, off, kw = dense(T, seed=11 + inner)
    alpha, beta = rand((Cch,), 3, 0.5, 1.5), rand((Cch,), 4, -0.1, 0.1)
    kw.update(alpha=alpha.to(DEV), beta=beta.to(DEV), Cch=Cch, inner=inner)
    check(T, "lif_soft", torch.uint8, x.to(DEV), x, off, T * N, kw, dict(alpha=alpha, beta=beta, inner=inner))


@pytest.mark.parametrize("T", [4, 3])
def test_add_with_a_period_shorter_than_the_row(T):
    x, off, kw = dense(T, seed=21)
    period = 64                                                  # 1028 = 16 * 64 + 4: the last period is cut
    add = rand((T, period), 5, -0.2, 0.2)
    kw.update(add=add.to(DEV), add_st=period, add_period=period)
    check(T, "lif_hard", torch.uint8, x.to(DEV), x, off, T * N, kw, dict(add=add, add_period=period))


@pytest.mark.parametrize("T", [5, 3])
def test_gather_with_negative_map_entries(T):
    rowlen, rows, nsrc = 4, N // 4, 300
    src = rand((nsrc, rowlen), 31)
    g = torch.Generator(device="cpu").manual_seed(32)
    rowmap = torch.randint(-40, nsrc, (T, rows), generator=g).clamp_(min=-1).to(torch.int32)
    assert int((rowmap < 0).sum()) > 10
    x_eff = torch.cat([src, torch.zeros(1, rowlen)])[rowmap.long()].reshape(T, N)      # (index -1: the zero row)
    off = torch.arange(T).view(T, 1) * N + torch.arange(N).view(1, N)
    kw = dict(args=(1, N, 0, 0, 0, N), rowmap=rowmap.reshape(-1).to(DEV), rowlen=rowlen)
    check(T, "lif_soft", torch.uint8, src.to(DEV), x_eff, off, T * N, kw)


@pytest.mark.parametrize("T,out_dtype", [(10, torch.uint8), (3, torch.float32)])
def test_two_problems_with_strides_larger_than_the_problem(T, out_dtype):
    """nrep = 2: the step and problem strides leave gaps (x and out differently), which must keep their sentinel."""
    nb, ni = 1, N
    x_sb, x_st, x_srep = 0, ni + 8, T * (ni + 8) + 16
    o_sb, o_st, o_srep = 0, ni + 12, T * (ni + 12) + 8
    xbuf = rand((2 * x_srep,), 41)
    t, pr, b, r = torch.meshgrid(torch.arange(T), torch.arange(2), torch.arange(nb), torch.arange(ni), indexing="ij")
    x_eff = xbuf[(pr * x_srep + b * x_sb + t * x_st + r)].reshape(T, 2 * N)
    off = (pr * o_srep + b * o_sb + t * o_st + r).reshape(T, 2 * N)
    kw = dict(args=(nb, ni, x_sb, x_st, o_sb, o_st), rep=(2, x_srep, o_srep))
    check(T, "if", out_dtype, xbuf.to(DEV), x_eff, off, 2 * o_srep, kw, problems=2 * nb)


def test_psn_and_glif_have_no_v_seq():
    x = torch.zeros((4, N), device=DEV)
    out, v = torch.empty((4, N), dtype=torch.uint8, device=DEV), torch.empty((4, N), device=DEV)
    psn = hip.NeuronParams("psn", psn_w=torch.eye(4, device=DEV), psn_b=torch.zeros(4, device=DEV))
    with hip.launch_log() as log:
        with pytest.raises(hip.SdfError) as e:
            hip.neuron_fwd(x, out, 4, 1, N, 0, N, 0, N, psn, v_seq=v)
        assert e.value.rc == hip.E_DTYPE
        with pytest.raises(hip.SdfError) as e:
            hip.neuron_fwd(x, out, 4, 1, N, 0, N, 0, N, hip.GlifParams(torch.zeros(9, device=DEV)), v_seq=v)
        assert e.value.rc == hip.E_DTYPE
    assert log.rows == []
