"""The general GLIF launch (sdf_glif_neuron_fwd: csrc/neuron.hip glif_neuron_kernel) and the GLIF token gate (sdf_qk_gate_glif_fwd:
csrc/qk_gate.hip) on the GPU, in every addressing form the eval plan of a GLIF model issues (engine_glif.py).

The reference in each case is `oracle.sdformer_oracle.glif_multistep` on the CPU, applied to the pre-activation the test forms
itself (the BN affine with `O.fma32`); the table handed to the kernel is the CPU-formed one (`table_of`: fp32 sigmoids of the CPU,
the products in the reference's order).  The assertion is bit equality, for fp32 and for u8 spikes.  Every output lies between two
256-byte guards, which must stay untouched, and every call is exactly one launch of the new kernel."""
import pytest
import torch

from oracle import sdformer_oracle as O
from sdformerflow_amd import hip
from test_glif_sltt_train_gpu import GATES, GG, SHAPES, case, logits, table_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 256, 0xA5
P = "spiking_neuron."


def rand(shape, seed, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def drawn_logits(T, seed):
    """Gate logits U(-1, 1) (gates ~ sigmoid: 0.27 .. 0.73, threshold ~ 0.5), as the fixtures' generator draws them."""
    return {k: rand((T,) if k == "conduct" else (), seed + i) for i, k in enumerate(GATES)}


def oracle_spikes(pre, lg):
    """(T, ...) fp32 pre-activation on the CPU -> (T, ...) u8 spikes of the reference recurrence."""
    s = O.glif_multistep(pre, {P + k: v for k, v in lg.items()}, P)
    return s.to(torch.uint8)


class Guarded:
    """A device buffer of `n` elements filled with 0xA5 bytes between two 256-byte guards of the same fill."""

    def __init__(self, n, dtype):
        self.size = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.size + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.size].view(dtype)

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all()) and bool((self.raw[GUARD + self.size:] == FILL).all())


def launch(kernel, fn):
    """fn() under the launch log: exactly one launch, of `kernel`."""
    with hip.launch_log() as log:
        fn()
    torch.cuda.synchronize()
    assert len(log.rows) == 1 and kernel in log.rows[0][0], [r[0] for r in log.rows]


def both_dtypes(n_out, call, want, pick=lambda t: t):
    """call(out) for an fp32 and a u8 output of n_out elements; pick(out) must equal `want` (u8, CPU) bit for bit."""
    for dtype in (torch.float32, torch.uint8):
        out = Guarded(n_out, dtype)
        launch("glif_neuron_kernel<", lambda: call(out.t))
        got = pick(out.t).cpu()
        assert got.dtype == dtype and torch.equal(got.to(torch.uint8), want), dtype
        assert bool(((got == 0) | (got == 1)).all()) and out.intact(), dtype


# ------------------------------------------------------------------ dense (T, N)
@pytest.mark.parametrize("T", [2, 4, 10])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_dense_equals_the_fixture_and_the_contiguous_kernel(T, tag):
    x0, _ = case(T, tag)
    N = x0[0].numel()
    want = torch.from_numpy(GG[f"T{T}_{tag}_s"]).reshape(T, N)
    tab = table_of(*logits(T).values())
    assert torch.equal(tab, torch.from_numpy(GG[f"T{T}_tab"]))
    assert torch.equal(oracle_spikes(x0, logits(T)).reshape(T, N), want)
    N4 = (N + 3) // 4 * 4                                               # (105 -> 108: the launch moves 4 neurons per lane)
    x = torch.zeros((T, N4))
    x[:, :N] = x0.reshape(T, N)
    xd, tabd = x.to(DEV), tab.to(DEV)
    both_dtypes(T * N4, lambda o: hip.glif_neuron_fwd(xd, o, T, 1, N4, 0, N4, 0, N4, tabd), want, lambda o: o.view(T, N4)[:, :N])
    s8 = torch.empty((T, N4), dtype=torch.uint8, device=DEV)
    hip.glif_neuron_fwd(xd, s8, T, 1, N4, 0, N4, 0, N4, tabd)
    assert torch.equal(s8, hip.glif_fwd(xd, tabd, torch.uint8)) and torch.equal(s8.float(), hip.glif_fwd(xd, tabd))


@pytest.mark.parametrize("T", [5, 20])
def test_dense_T5_T20_with_a_ragged_last_workgroup(T):
    N = 1028                                                            # 257 quads: two workgroups, one lane in the second
    lg = drawn_logits(T, 500 + T)
    x = 3.0 * rand((T, N), 40 + T, -0.3, 0.6)
    want = oracle_spikes(x, lg)
    assert 0.05 < float(want.float().mean()) < 0.95
    xd, tabd = x.to(DEV), table_of(*lg.values()).to(DEV)
    both_dtypes(T * N, lambda o: hip.glif_neuron_fwd(xd, o, T, 1, N, 0, N, 0, N, tabd), want, lambda o: o.view(T, N))


# ------------------------------------------------------------------ channel-last activation with the eval-BN affine (engine._neuron_bd)
@pytest.mark.parametrize("shape", [(2, 10, 3, 5, 36), (1, 2, 3, 5, 36)])
def test_channel_last_with_bn_over_the_last_dim(shape):
    B, D, h, w, Cc = shape
    lg = drawn_logits(D, 600 + D)
    x, a, b = 2.0 * rand(shape, 61, -0.3, 0.6), rand((Cc,), 62, 0.5, 1.5), rand((Cc,), 63, -0.2, 0.2)
    want = oracle_spikes(O.fma32(x, a, b).permute(1, 0, 2, 3, 4).contiguous(), lg)          # (D, B, h, w, C)
    assert 0.05 < float(want.float().mean()) < 0.95
    xd, ad, bd, tabd = x.to(DEV), a.to(DEV), b.to(DEV), table_of(*lg.values()).to(DEV)
    n = h * w * Cc
    both_dtypes(x.numel(), lambda o: hip.glif_neuron_fwd(xd, o, D, B, n, D * n, n, D * n, n, tabd, alpha=ad, beta=bd, Cch=Cc, inner=1),
                want, lambda o: o.view(shape).permute(1, 0, 2, 3, 4))


def test_channel_planes_with_bn_inner_above_one():
    T, B, Cc, H, W = 4, 2, 8, 3, 4
    lg = drawn_logits(T, 640)
    x, a, b = 2.0 * rand((T, B, Cc, H, W), 64, -0.3, 0.6), rand((Cc,), 65, 0.5, 1.5), rand((Cc,), 66, -0.2, 0.2)
    want = oracle_spikes(O.fma32(x, a.view(1, 1, Cc, 1, 1), b.view(1, 1, Cc, 1, 1)), lg)
    assert 0.05 < float(want.float().mean()) < 0.95
    xd, ad, bd, tabd = x.to(DEV), a.to(DEV), b.to(DEV), table_of(*lg.values()).to(DEV)
    n = Cc * H * W
    both_dtypes(x.numel(), lambda o: hip.glif_neuron_fwd(xd, o, T, B, n, n, B * n, n, B * n, tabd, alpha=ad, beta=bd, Cch=Cc, inner=H * W),
                want, lambda o: o.view(T, B, Cc, H, W))


# ------------------------------------------------------------------ row-map gather with the positional add (the attention's neurons)
def test_gather_through_a_row_map_with_padding_rows_and_a_periodic_add():
    T, rows, L, src_rows, prows = 2, 26, 96, 40, 9
    lg = drawn_logits(T, 700)
    src = 2.0 * rand((src_rows, L), 71, -0.3, 0.6)
    add = rand((T, prows, L), 72, -0.3, 0.3)
    m = torch.randint(0, src_rows, (T, rows), generator=torch.Generator().manual_seed(73), dtype=torch.int32)
    m[0, 3], m[1, 3], m[0, 4], m[0, 25], m[1, 0] = 7, 7, 7, 39, 39                          # repeated rows, within and across steps
    pad = [(0, 0), (0, 11), (1, 11), (1, 17), (1, 25)]                                    # five padding entries
    for t, r in pad:
        m[t, r] = -1
    gathered = torch.cat([src, torch.zeros(1, L)])[torch.where(m < 0, src_rows, m).long()]          # (T, rows, L); -1 reads 0.0
    period = add[:, torch.arange(rows) % prows]                                                     # (T, rows, L)
    want = oracle_spikes(gathered + period, lg)
    assert 0.05 < float(want.float().mean()) < 0.95
    # row 11 is padding at both steps: its spikes are those of x = 0 under the add
    assert torch.equal(want[:, 11], oracle_spikes(torch.zeros(T, L) + period[:, 11], lg))
    sd, addd, md, tabd = src.to(DEV), add.to(DEV), m.reshape(-1).to(DEV), table_of(*lg.values()).to(DEV)
    n = rows * L
    both_dtypes(T * n, lambda o: hip.glif_neuron_fwd(sd, o, T, 1, n, 0, 0, 0, n, tabd, rowmap=md, rowlen=L, add=addd, add_st=prows * L,
                                                     add_period=prows * L), want, lambda o: o.view(T, rows, L))
    # without the add the padding rows are the spikes of x = 0 alone
    want0 = oracle_spikes(gathered, lg)
    assert torch.equal(want0[:, 11], oracle_spikes(torch.zeros(T, L), lg))
    both_dtypes(T * n, lambda o: hip.glif_neuron_fwd(sd, o, T, 1, n, 0, 0, 0, n, tabd, rowmap=md, rowlen=L), want0, lambda o: o.view(T, rows, L))


# ------------------------------------------------------------------ channel-slice output (engine._decoder_image)
def test_channel_slice_output_with_the_batch_as_the_outer_dimension():
    B, D, hw, take, pitch, cp, c0 = 2, 5, 7, 20, 24, 64, 8
    lg = drawn_logits(D, 800)
    src = 2.0 * rand((B, D, hw, pitch), 81, -0.3, 0.6)
    want = oracle_spikes(src[..., :take].permute(1, 0, 2, 3).contiguous(), lg)             # (D, B, hw, take)
    assert 0.05 < float(want.float().mean()) < 0.95
    sd, tabd = src.to(DEV), table_of(*lg.values()).to(DEV)
    img = Guarded(B * D * hw * cp, torch.uint8)
    launch("glif_neuron_kernel<", lambda: hip.glif_neuron_fwd(sd, img.t[c0:], D, hw, take, pitch, hw * pitch, cp, hw * cp, tabd,
                                                              rep=(B, D * hw * pitch, D * hw * cp)))
    got = img.t.view(B, D, hw, cp).cpu()
    assert torch.equal(got[..., c0:c0 + take].permute(1, 0, 2, 3), want)
    assert bool((got[..., :c0] == FILL).all()) and bool((got[..., c0 + take:] == FILL).all()) and img.intact()
    # the per-sample form the engine issues (no outer dimension) writes the same bytes
    one = Guarded(B * D * hw * cp, torch.uint8)
    for b in range(B):
        hip.glif_neuron_fwd(sd[b], one.t.view(B, -1)[b][c0:], D, hw, take, pitch, hw * pitch, cp, hw * cp, tabd)
    assert torch.equal(one.t, img.t) and one.intact()


# ------------------------------------------------------------------ the token gate
# Gate node of the gate cases: c = 1 - b (1 - sigmoid(conduct)) = 0.75 and th = sigmoid(1.5) = 0.82, so one spike in a head (u = 0.74)
# does not fire a resting gate and two do; a short memory (L = 0.56) and a strong reset (g = 0.88) keep that so at the later steps.
# q at density 0.05 gives head sums of mean 1.6.  With dense q every head sum exceeds th < 1 and every gate fires: the test would
# prove nothing, hence the asserted 20 % .. 80 % band at every step (0.40 .. 0.69 on the CPU reference over all cases).
GATE_DENSITY = 0.05


def gate_logits(Tq):
    z = torch.zeros(())
    return {"alpha": z, "beta": z, "gamma": torch.tensor(2.0), "tau": torch.tensor(-2.0), "v_threshold": torch.tensor(1.5),
            "linear_decay": torch.tensor(-4.0), "v_subreset": torch.tensor(2.0), "conduct": torch.zeros(Tq)}


@pytest.mark.parametrize("Tq", [2, 4])
@pytest.mark.parametrize("rows", [7, 1000])
@pytest.mark.parametrize("Cc", [96, 192])
def test_token_gate(Tq, rows, Cc):
    G, lg = Cc // 32, gate_logits(Tq)
    g = torch.Generator().manual_seed(900 + Tq + rows + Cc)
    q = (torch.rand((Tq, rows, Cc), generator=g) < GATE_DENSITY).to(torch.uint8)
    k = (torch.rand((Tq, rows, Cc), generator=g) < 0.5).to(torch.uint8)
    a = q.view(Tq, rows, G, 32).sum(-1, dtype=torch.float32)
    A = oracle_spikes(a, lg)                                                               # (Tq, rows, G)
    rates = A.float().flatten(1).mean(1)
    assert bool(((rates >= 0.2) & (rates <= 0.8)).all()), rates
    want = k * A.repeat_interleave(32, dim=-1)
    tabd = table_of(*lg.values()).to(DEV)
    qk = torch.cat([q, k], -1).to(DEV)                                                     # the two halves of one (Tq, rows, 2C) buffer
    forms = [(q.to(DEV), k.to(DEV), Cc), (qk[..., :Cc], qk[..., Cc:], 2 * Cc)]
    for qd, kd, ld in forms:
        for with_gate in (False, True):
            e, gt = Guarded(Tq * rows * Cc, torch.uint8), Guarded(Tq * rows * G, torch.uint8)
            launch("qk_gate_glif_kernel<", lambda: hip.qk_gate_glif(qd, kd, e.t, Tq, rows, Cc, tabd, ldq=ld, ldk=ld,
                                                                    gate=gt.t if with_gate else None))
            assert torch.equal(e.t.view(Tq, rows, Cc).cpu(), want) and e.intact(), (ld, with_gate)
            assert gt.intact()
            if with_gate:
                assert torch.equal(gt.t.view(Tq, rows, G).cpu(), A)
            else:
                assert bool((gt.t == FILL).all())
