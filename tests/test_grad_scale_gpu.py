"""The scaled tail of the training step on the GPU (csrc/grad_step.hip): the in-place scale bit for bit, the coefficient kernel with
the loss scaler against sdf_grad_clip_coef and the scale-update restatement, the scaled AdamW kernel (a skipped step writes nothing;
scale 1 is sdf_adamw_step bit for bit; a real scale within twice torch's own fp32 distance from the fp64 restatement), and three loops
beside their torch.amp.GradScaler / clip_grad_norm_ / AdamW(foreach=False) twins: eight scaled steps with one non-finite gradient,
gradient accumulation over seven micro-steps, and one fp16 train_step of the smallest model."""
import copy

import numpy as np
import pytest
import torch

from sdformerflow_amd import hip, train
from test_grad_step_gpu import (BETAS, DEV, EPS, GUARD, INACTIVE, LENGTHS, LR, OFFSETS, TOTAL, carve, deterministic_convolutions,  # noqa: F401
                                guarded, guards_intact, kname, make_values, ulp32)
from test_grad_scale_cpu import TRAJECTORY, torch_scaler_trajectory

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
NSEG = len(LENGTHS)


def shifted(shift, n=TOTAL):
    """(outer, off, flat): n floats `shift` floats off a 16-byte boundary, between guard bytes."""
    outer, off = guarded((n + shift) * 4)
    flat = carve(outer, off, torch.float32, n + shift)[shift:]
    assert flat.data_ptr() % 16 == 4 * shift
    return outer, off, flat


def set_state(state, **kw):
    v = hip.loss_scale_views(state)
    for k, x in kw.items():
        v[k].fill_(x)


# ------------------------------------------------------------------------------------------------ grad_scale
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_grad_scale_in_place(shift):
    """g * c in one fp32 multiplication per element, equal to numpy's product byte for byte - normal values, denormals (as operands
    and, with c = -2^-100, as results), signed zeros, inf, -inf and NaN; the inactive segment, the float(s) in front of the shifted
    buffer and the guard bytes keep their bytes; one launch of the scale kernel."""
    seg = hip.GradSegments(zip(OFFSETS, LENGTHS), DEV)
    mask_host = np.ones(NSEG, dtype=np.uint8)
    mask_host[INACTIVE] = 0
    mask = torch.from_numpy(mask_host).to(DEV)
    outer, off, flat = shifted(shift)
    for seed, c in ((21, 0.3712), (22, -2.0 ** -100), (23, 1.0)):
        g = make_values(seed)
        if seed == 22:
            g[OFFSETS[-1] + 17:OFFSETS[-1] + 4000] *= np.float32(2.0 ** 90)             # products on both sides of the denormal range
        flat.copy_(torch.from_numpy(g))
        coef = torch.tensor([c], dtype=torch.float32, device=DEV)
        with np.errstate(all="ignore"):
            want = g * np.float32(c)
        o, n = OFFSETS[INACTIVE], LENGTHS[INACTIVE]
        want[o:o + n] = g[o:o + n]
        with hip.launch_log() as log:
            assert hip.grad_scale(flat, seg, coef, mask) is flat
        torch.cuda.synchronize()
        assert [(kname(r[0]), r[1], r[2]) for r in log.rows] == [("grad_scale_kernel", 128 * NSEG, 256)], log.rows
        got = flat.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (shift, c, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert guards_intact(outer, off, (TOTAL + shift) * 4) and bool((outer[off:off + 4 * shift] == GUARD).all())
    # no mask: every segment
    g = make_values(25)
    flat.copy_(torch.from_numpy(g))
    hip.grad_scale(flat, seg, torch.tensor([0.5], device=DEV))
    with np.errstate(all="ignore"):
        assert flat.cpu().numpy().tobytes() == (g * np.float32(0.5)).tobytes()


# ------------------------------------------------------------------------------------------------ grad_clip_scale_coef
def stats_table(scale=1.0, seed=3):
    g = make_values(seed)
    g[~np.isfinite(g)] = 0.5
    return hip.grad_stats(torch.from_numpy((g * np.float32(scale)).astype(np.float32)).to(DEV), hip.GradSegments(zip(OFFSETS, LENGTHS), DEV))


@pytest.mark.parametrize("scale,max_norm", [(1.0, 100.0), (1e-3, 100.0), (1.0, 0.125), (1.0, float("inf"))])
def test_clip_scale_coef_equals_clip_coef(scale, max_norm):
    """clip_unscaled = 0: coef and record are sdf_grad_clip_coef's, byte for byte, whatever the loss scale is; clip_unscaled = 1: the
    fp64 formula on total * inv_scale, to one fp32 rounding."""
    table = stats_table(scale)
    for mask in (None, [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]):
        m = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=DEV)
        coef0, record0 = hip.grad_clip_coef(table, max_norm, m)
        for s in (1.0, 65536.0, 3.0):
            state = hip.loss_scale_state(s, 0, DEV)
            c_outer, c_off = guarded(4)
            r_outer, r_off = guarded(16)
            with hip.launch_log() as log:
                coef, record = hip.grad_clip_scale_coef(table, max_norm, state, mask=m, coef=carve(c_outer, c_off, torch.float32, 1),
                                                        record=carve(r_outer, r_off, torch.float64, 2))
            torch.cuda.synchronize()
            assert [(kname(r[0]), r[1], r[2]) for r in log.rows] == [("grad_clip_scale_coef_kernel", 1, 256)], log.rows
            assert guards_intact(c_outer, c_off, 4) and guards_intact(r_outer, r_off, 16)
            assert coef.cpu().numpy().tobytes() == coef0.cpu().numpy().tobytes() and record.cpu().numpy().tobytes() == record0.cpu().numpy().tobytes()
            st = hip.loss_scale_read(state)
            inv = float(np.float32(1.0 / np.float64(np.float32(s))))
            assert st == {"scale": s, "growth_tracker": 1, "inv_scale": inv, "found_inf": 0, "skipped": 0}
            coef_u, record_u = hip.grad_clip_scale_coef(table, max_norm, state, mask=m, clip_unscaled=True, update=False)
            want = min(1.0, max_norm / (float(record0[0]) * inv + 1e-6))
            print(f"scale {scale} max_norm {max_norm} mask {mask is not None} loss scale {s}: coef {float(coef)!r}, unscaled {float(coef_u)!r} (fp64 formula {want!r})")
            assert abs(float(coef_u) - want) <= 2.0 ** -23 * want and record_u.cpu().numpy().tobytes() == record0.cpu().numpy().tobytes()


def test_clip_scale_coef_state_transitions():
    """The trajectory of test_grad_scale_cpu.py (growth, a growth that would overflow, backoff, two non-finite steps in a row) through
    the kernel: scale and tracker equal the restatement - and torch.amp.GradScaler on the GPU - after every step; found_inf, inv_scale
    and skipped are those of the step; update = 0 leaves scale and tracker alone and still gives the verdict."""
    table = stats_table()
    init = 2.0 ** 126
    want_torch = torch_scaler_trajectory(DEV, init, TRAJECTORY, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    s_outer, s_off = guarded(24)
    state = carve(s_outer, s_off, torch.int64, 3)
    state.copy_(hip.loss_scale_state(init, 0, DEV))
    scale, tracker, skipped = init, 0, 0
    for f, wt in zip(TRAJECTORY, want_torch):
        table[5, 4] = float(2 * f)
        _, record = hip.grad_clip_scale_coef(table, 100.0, state, 2.0, 0.5, 2)
        carried = scale
        scale, tracker = train.loss_scale_restatement(scale, tracker, f, 2.0, 0.5, 2)
        skipped += f
        st = hip.loss_scale_read(state)
        assert st == {"scale": scale, "growth_tracker": tracker, "inv_scale": float(np.float32(1.0 / np.float64(carried))), "found_inf": f,
                      "skipped": skipped}, (f, st)
        assert (st["scale"], st["growth_tracker"]) == wt and float(record[1]) == 2.0 * f
    assert guards_intact(s_outer, s_off, 24) and skipped == 3
    for f in (1, 0):
        table[5, 4] = float(f)
        hip.grad_clip_scale_coef(table, 100.0, state, 2.0, 0.5, 2, update=False)
        skipped += f
        st = hip.loss_scale_read(state)
        assert (st["scale"], st["growth_tracker"], st["found_inf"], st["skipped"]) == (scale, tracker, f, skipped)


# ------------------------------------------------------------------------------------------------ adamw_step_scaled
class Packed:
    """p, g, m, v of the packed lengths on the GPU, the three flat buffers one float off a 16-byte boundary between guard bytes.
    `mirror`: the parameters are packed like the bucket; `own`: every parameter starts on its own 16-byte boundary."""

    def __init__(self, layout, p, m, v):
        self.p_offs = OFFSETS if layout == "mirror" else tuple(int(x) for x in np.cumsum([0] + [(n + 3) // 4 * 4 + 4 for n in LENGTHS[:-1]]))
        self.p_total = self.p_offs[-1] + LENGTHS[-1]
        self.shift, self.p_shift = 1, 1 if layout == "mirror" else 0
        self.outers = {k: guarded((TOTAL + self.shift) * 4) for k in "gmv"}
        self.outers["p"] = guarded((self.p_total + self.p_shift) * 4)
        self.flat = {k: carve(o, off, torch.float32, TOTAL + self.shift)[self.shift:] for k, (o, off) in self.outers.items() if k != "p"}
        self.pbuf = carve(*self.outers["p"], torch.float32, self.p_total + self.p_shift)[self.p_shift:]
        self.pbuf.fill_(-7.5)                                                # (the padding between `own` parameters)
        for o, po, n in zip(OFFSETS, self.p_offs, LENGTHS):
            self.pbuf[po:po + n] = torch.from_numpy(p[o:o + n]).to(DEV)
        self.flat["m"].copy_(torch.from_numpy(m))
        self.flat["v"].copy_(torch.from_numpy(v))
        self.rows = hip.adamw_rows(NSEG)
        self.rows["offset"], self.rows["length"], self.rows["active"] = OFFSETS, LENGTHS, 1
        self.rows["active"][INACTIVE] = 0
        self.rows["param"] = [self.pbuf.data_ptr() + 4 * po for po in self.p_offs]

    def scalars(self, step, wd):
        for name, val in zip(("decay", "w1", "beta2", "w2", "neg_step_size", "bc2_sqrt", "eps"), train.adamw_scalars(step, LR, BETAS, EPS, wd)):
            self.rows[name] = val

    def snapshot(self):
        """every byte the kernel could reach: the four guarded allocations"""
        torch.cuda.synchronize()
        return {k: o.cpu().numpy().copy() for k, (o, _) in self.outers.items()}

    def values(self):
        host = self.pbuf.cpu().numpy()
        return np.concatenate([host[o:o + n] for o, n in zip(self.p_offs, LENGTHS)]), self.flat["m"].cpu().numpy(), self.flat["v"].cpu().numpy()


def adamw_inputs(seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(TOTAL).astype(np.float32)
    p[rng.choice(TOTAL, 50, replace=False)] = 0.0
    m = (0.1 * rng.standard_normal(TOTAL)).astype(np.float32)
    v = (0.01 * rng.random(TOTAL)).astype(np.float32)
    g = make_values(seed)
    g[~np.isfinite(g)] = 0.0
    return p, g, m, v


@pytest.mark.parametrize("layout", ["mirror", "own"])
def test_adamw_scaled_skips_and_equals_the_unscaled_kernel(layout):
    """found_inf = 1: every byte of p, m, v and of the guards around them is what it was.  found_inf = 0 and inv_scale = 1: the bytes
    sdf_adamw_step writes from the same inputs (x * 1 is x), with and without a clip coefficient."""
    p, g, m, v = adamw_inputs(31)
    coef = torch.tensor([0.3712], dtype=torch.float32, device=DEV)
    for step, wd, c in ((1, 0.0, None), (7, 0.01, coef)):
        a, b = Packed(layout, p, m, v), Packed(layout, p, m, v)
        for k in (a, b):
            k.flat["g"].copy_(torch.from_numpy(g))
            k.scalars(step, wd)
        state = hip.loss_scale_state(65536.0, 0, DEV)
        set_state(state, found_inf=1)
        before = b.snapshot()
        with hip.launch_log() as log:
            hip.adamw_step_scaled(b.flat["g"], b.flat["m"], b.flat["v"], b.rows, state, None, c)
        assert [(kname(r[0]), r[1], r[2]) for r in log.rows] == [("adamw_step_scaled_kernel", 128 * NSEG, 256)], log.rows
        after = b.snapshot()
        assert all(before[k].tobytes() == after[k].tobytes() for k in before)
        set_state(state, found_inf=0, inv_scale=1.0)
        hip.adamw_step(a.flat["g"], a.flat["m"], a.flat["v"], a.rows, None, c)
        hip.adamw_step_scaled(b.flat["g"], b.flat["m"], b.flat["v"], b.rows, state, None, c)
        va, vb = a.values(), b.values()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(va, vb)) and va[0].tobytes() != p.tobytes()
        for k in (a, b):
            assert all(guards_intact(o, off, (TOTAL + k.shift) * 4) for n, (o, off) in k.outers.items() if n != "p")
            assert guards_intact(*k.outers["p"], (k.p_total + k.p_shift) * 4)
        assert a.pbuf.cpu().numpy().tobytes() == b.pbuf.cpu().numpy().tobytes()                # (the padding too)
        assert hip.loss_scale_read(state)["scale"] == 65536.0                                    # the state is only read


def torch_adamw_scaled_cpu(p, g, m, v, step0, wd, coef, inv):
    """torch.optim.AdamW(foreach=False) on CPU fp32 tensors, one step from (m, v, step0) on the gradient (g * coef) * inv - two fp32
    multiplications, as clip_grad_norm_ followed by GradScaler.unscale_ performs."""
    ps = [torch.nn.Parameter(torch.from_numpy(p[o:o + n].copy())) for o, n in zip(OFFSETS, LENGTHS)]
    opt = torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    for i, (q, o, n) in enumerate(zip(ps, OFFSETS, LENGTHS)):
        if i == INACTIVE:
            continue
        q.grad = torch.from_numpy(g[o:o + n].copy()).mul_(torch.tensor(coef, dtype=torch.float32)).mul_(torch.tensor(inv, dtype=torch.float32))
        opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(m[o:o + n].copy()),
                        "exp_avg_sq": torch.from_numpy(v[o:o + n].copy())}
    opt.step()
    out = [a.copy() for a in (p, m, v)]
    for i, (q, o, n) in enumerate(zip(ps, OFFSETS, LENGTHS)):
        if i != INACTIVE:
            out[0][o:o + n], out[1][o:o + n], out[2][o:o + n] = q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()
    return out


@pytest.mark.parametrize("layout", ["mirror", "own"])
def test_adamw_scaled_kernel(layout):
    """Gradients that carry a loss scale of 2^16, a clip coefficient and inv_scale = 2^-16: d = the largest elementwise distance of
    torch's fp32 AdamW(foreach=False) on the CPU, fed (g * c) * inv_scale, from the fp64 restatement; the kernel may be 2 d from the
    restatement, or one ulp of the value where that is more.  Step 1 from zero moments, step 1001 from a long-trained state."""
    coef, inv, wd = float(np.float32(0.3712)), 2.0 ** -16, 0.01
    p, g, m, v = adamw_inputs(41)
    g = (g * np.float32(65536.0)).astype(np.float32)
    state = hip.loss_scale_state(65536.0, 0, DEV)
    assert hip.loss_scale_read(state)["inv_scale"] == inv
    coef_dev = torch.tensor([coef], dtype=torch.float32, device=DEV)
    for step, (m0, v0) in ((1, (np.zeros_like(m), np.zeros_like(v))), (1001, (m, v))):
        k = Packed(layout, p, m0, v0)
        k.flat["g"].copy_(torch.from_numpy(g))
        k.scalars(step, wd)
        hip.adamw_step_scaled(k.flat["g"], k.flat["m"], k.flat["v"], k.rows, state, None, coef_dev)
        got = k.values()
        want = [np.concatenate(x) for x in zip(*[train.adamw_restatement(p[o:o + n], g[o:o + n].astype(np.float64) * inv, m0[o:o + n], v0[o:o + n], step, LR, BETAS, EPS, wd, coef)
                                                 if i != INACTIVE else (p[o:o + n].astype(np.float64), m0[o:o + n].astype(np.float64), v0[o:o + n].astype(np.float64))
                                                 for i, (o, n) in enumerate(zip(OFFSETS, LENGTHS))])]
        ref = torch_adamw_scaled_cpu(p, g, m0, v0, step - 1, wd, coef, inv)
        for name, a, w, r in zip("pmv", got, want, ref):
            d = float(np.abs(r.astype(np.float64) - w).max())
            err = np.abs(a.astype(np.float64) - w)
            print(f"{layout} step {step} {name}: torch d {d:.3e}, kernel {err.max():.3e}, differs from torch in {int((a != r).sum())} of {a.size}")
            assert (err <= np.maximum(2.0 * d, ulp32(w))).all(), (name, step, float(err.max()), d)
        o, n = OFFSETS[INACTIVE], LENGTHS[INACTIVE]
        assert all(a[o:o + n].tobytes() == b[o:o + n].tobytes() for a, b in zip(got, (p, m0, v0)))
        assert k.flat["g"].cpu().numpy().tobytes() == g.tobytes()
        assert all(guards_intact(o, off, (TOTAL + k.shift) * 4) for nm, (o, off) in k.outers.items() if nm != "p")
        assert guards_intact(*k.outers["p"], (k.p_total + k.p_shift) * 4)


# ------------------------------------------------------------------------------------------------ loops beside their torch twins
def three_linears():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 6), torch.nn.Tanh(), torch.nn.Linear(6, 32)).to(DEV)


def np64(t):
    return t.detach().double().cpu().numpy().ravel()


class TwoD:
    """The `2 d` rule over a step of a model and its torch twin: before(): both states; after(): the kernel's distance from the fp64
    restatement of ITS inputs within twice the distance of torch's result from the restatement of the twin's (floor: one ulp)."""

    def __init__(self, model, opt, twin, topt, lr, wd):
        self.model, self.opt, self.twin, self.topt, self.lr, self.wd = model, opt, twin, topt, lr, wd

    def before(self):
        self.mine = {p: (np64(p), np64(self.opt.state[p]["exp_avg"]), np64(self.opt.state[p]["exp_avg_sq"])) for p in self.model.parameters()}
        self.theirs = {}
        for p in self.twin.parameters():
            st = self.topt.state.get(p, {})
            z = np.zeros(p.numel())
            self.theirs[p] = (np64(p), np64(st["exp_avg"]) if "exp_avg" in st else z, np64(st["exp_avg_sq"]) if "exp_avg_sq" in st else z)

    def after(self, step, my_grads, coef, inv, their_grads, label):
        """my_grads: {p: what the buckets held (still scaled, not clipped)}; their_grads: {p: the gradient torch stepped on}."""
        d, errs = 0.0, []
        for p in self.twin.parameters():
            if their_grads.get(p) is None:
                continue
            want = train.adamw_restatement(*self.theirs[p][:1], their_grads[p], *self.theirs[p][1:], step, self.lr, BETAS, EPS, self.wd)[0]
            d = max(d, float(np.abs(np64(p) - want).max()))
        for p in self.model.parameters():
            if my_grads.get(p) is None:
                continue
            want = train.adamw_restatement(*self.mine[p][:1], my_grads[p] * inv, *self.mine[p][1:], step, self.lr, BETAS, EPS, self.wd, coef)[0]
            errs.append((np.abs(np64(p) - want), ulp32(want)))
        worst = max(float(e.max()) for e, _ in errs)
        print(f"{label}: torch's distance from the fp64 restatement d {d:.3e}; the kernel's {worst:.3e}")
        for e, u in errs:
            assert (e <= np.maximum(2.0 * d, u)).all(), (label, float(e.max()), d)


def test_scaled_steps_beside_a_torch_twin():
    """Eight steps of three Linear layers with growth_interval 2 and an inf written into one gradient at step 3, in the reference's
    order - scale, backward, clip_grad_norm_ on the STILL-SCALED gradients, scaler.step, scaler.update - with torch.amp.GradScaler +
    AdamW(foreach=False) beside LossScaler + BucketAdamW.  Same verdicts, the same scale and tracker after every step, parameters within
    the 2 d rule at every step that ran.  The host counts the skipped step first and takes it back when it reads the verdict, at the
    start of the next step(): every later count equals torch's, and nothing here asks for a reconciliation."""
    lr, wd, clip = 1e-2, 0.01, 100.0
    model = three_linears()
    twin = copy.deepcopy(model)
    buckets = train.GradientBuckets(model.parameters())
    opt = train.BucketAdamW(buckets, lr, weight_decay=wd)
    scaler = train.LossScaler(growth_interval=2, device=DEV)
    topt = torch.optim.AdamW(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    ts = torch.amp.GradScaler("cuda", growth_interval=2)
    rule = TwoD(model, opt, twin, topt, lr, wd)
    tpar = dict(zip(model.parameters(), twin.parameters()))
    gen = torch.Generator().manual_seed(9)
    ran = 0
    for step in range(1, 9):
        x, y = torch.randn(16, 5, generator=gen).to(DEV), torch.randn(16, 32, generator=gen).to(DEV)
        rule.before()
        topt.zero_grad()
        ts.scale((twin(x) - y).square().mean()).backward()
        if step == 3:
            twin[2].weight.grad[1, 2] = float("inf")
        torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)
        t_start = [p.detach().clone() for p in twin.parameters()]
        ts.step(topt)
        ts.update()
        t_skipped = all(torch.equal(a, b) for a, b in zip(t_start, twin.parameters()))

        buckets.begin()
        scaler.scale((model(x) - y).square().mean()).backward()
        buckets.finish()
        if step == 3:
            model[2].weight.grad[1, 2] = float("inf")
        start = [p.detach().clone() for p in model.parameters()]
        with hip.launch_log() as log:
            opt.step(clip, scaler=scaler)
        nb = len(buckets.flat)
        assert [kname(r[0]) for r in log.rows] == ["grad_stats_partial_kernel", "grad_stats_finish_kernel"] * nb + ["grad_clip_scale_coef_kernel"] + ["adamw_step_scaled_kernel"] * nb
        st = hip.loss_scale_read(scaler.state)
        skipped = bool(st["found_inf"])
        assert skipped == t_skipped == (step == 3)
        assert scaler.state_dict() == ts.state_dict(), (step, scaler.state_dict(), ts.state_dict())
        if skipped:
            assert all(torch.equal(a, b) for a, b in zip(start, model.parameters()))
            assert all(float(opt.state[p]["step"]) == ran + 1 for p in model.parameters())          # counted; the verdict is still unread
        else:
            ran += 1
            _, (total, bad), coef = opt.stats.read()
            assert bad == 0.0 and coef < 1.0                                                         # the clip bounds the scaled norm
            rule.after(ran, {p: np64(buckets._views[p]) for p in model.parameters()}, coef, st["inv_scale"],
                       {tp: np64(tp.grad) for tp in twin.parameters()}, f"step {step}")
            assert all(float(opt.state[p]["step"]) == float(topt.state[tpar[p]]["step"]) == ran for p in model.parameters()), step
    assert scaler.skipped == 1 and ran == 7
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert all(float(sd["state"][i]["step"]) == float(tsd["state"][i]["step"]) == 7.0 for i in tsd["state"])
    # a disabled scaler only skips: the scale stays 1
    off = train.LossScaler(enabled=False, device=DEV)
    for bad_step in (False, True):
        buckets.begin()
        off.scale((model(x) - y).square().mean()).backward()
        buckets.finish()
        if bad_step:
            model[0].bias.grad[0] = float("nan")
        start = [p.detach().clone() for p in model.parameters()]
        opt.step(clip, scaler=off)
        assert all(torch.equal(a, b) for a, b in zip(start, model.parameters())) == bad_step
        assert off.get_scale() == 1.0 and hip.loss_scale_read(off.state)["growth_tracker"] == 0
    assert off.skipped == 1 and all(float(opt.state[p]["step"]) == 8.0 for p in model.parameters())


def test_accumulation_beside_a_torch_twin():
    """num_acc = 3 over seven micro-steps (two full groups and a remainder of one, stepped because it is the last) through train_step,
    beside the reference's loop written out with torch: loss / num_acc, backward into the running sum, clip_grad_norm_ on the sum IN
    PLACE after every micro-step, step and zero on (i + 1) % 3 == 0 or the last.  After every micro-step the buckets (times the
    coefficient where the update applies it instead of writing it) are within 64 * 2^-24 of torch's clipped sums, relative to the
    tensor's largest element: torch takes the norm in fp32 (test_grad_step_cpu.py holds its coefficient to that bound), every term
    of an element's sum carries its own coefficient's error, and the sum may cancel.  The three updates obey the 2 d rule."""
    lr, wd, clip, num_acc, n_micro = 1e-2, 0.01, 0.01, 3, 7          # (a micro-step's gradient norm is about 0.018: the clip acts)
    model = three_linears()
    twin = copy.deepcopy(model)
    buckets = train.GradientBuckets(model.parameters())
    opt = train.BucketAdamW(buckets, lr, weight_decay=wd)
    topt = torch.optim.AdamW(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    rule = TwoD(model, opt, twin, topt, lr, wd)
    tpar = dict(zip(model.parameters(), twin.parameters()))
    gen = torch.Generator().manual_seed(12)
    fwd = lambda net, x: [net(x).view(-1, 2, 4, 4)]
    mask = torch.ones(4, 1, 4, 4, device=DEV)
    steps, clipped = 0, 0
    rule.before()
    for i in range(n_micro):
        x, label = torch.randn(4, 5, generator=gen).to(DEV), torch.randn(4, 2, 4, 4, generator=gen).to(DEV)
        step_now = (i + 1) % num_acc == 0 or i + 1 == n_micro
        t_loss = train.flow_loss_supervised(fwd(twin, x), label, mask) / num_acc
        t_loss.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)
        t_grads = {tp: np64(tp.grad) for tp in twin.parameters()}
        with hip.launch_log() as log:
            loss = train.train_step(model, opt, x, label, mask, buckets=buckets, clip_grad=clip, forward_fn=fwd, num_acc=num_acc, step_now=step_now)
        kernels = [kname(r[0]) for r in log.rows]
        nb = len(buckets.flat)
        tail = ["grad_stats_partial_kernel", "grad_stats_finish_kernel"] * nb + ["grad_clip_coef_kernel"]
        assert kernels[-(3 * nb + 1):] == tail + (["adamw_step_kernel"] if step_now else ["grad_scale_kernel"]) * nb, kernels
        assert abs(float(loss) - float(t_loss.detach())) <= 1e-6 * abs(float(t_loss.detach()))
        _, _, coef = opt.stats.read()
        clipped += coef < 1.0
        for p in model.parameters():
            mine = np64(buckets._views[p]) * (coef if step_now else 1.0)
            want = t_grads[tpar[p]]
            assert np.abs(mine - want).max() <= 64 * U24 * np.abs(want).max(), (i, float(np.abs(mine - want).max()), float(np.abs(want).max()))
        if step_now:
            steps += 1
            topt.step()
            rule.after(steps, {p: np64(buckets._views[p]) for p in model.parameters()}, coef, 1.0, t_grads, f"micro-step {i}")
            topt.zero_grad()
            assert all(float(opt.state[p]["step"]) == steps for p in model.parameters())
            rule.before()
        assert buckets.accumulating == (not step_now)
    assert steps == 3 and clipped == n_micro


@pytest.mark.parametrize("init_scale", [65536.0, 64.0])
def test_fp16_train_step_beside_a_torch_twin(deterministic_convolutions, init_scale):
    """One train_step(amp="fp16", scaler=...) of the smallest model test_train_gpu.py trains, beside a twin from the same weights and
    inputs taken through forward_train and flow_loss_supervised under fp16 autocast with torch's GradScaler, clip_grad_norm_ on the
    still-scaled gradients and AdamW.  Both agree on skip or step and on the scale afterwards; a step that ran obeys the 2 d rule, a
    skipped one leaves every parameter bit-equal to the start.  A second step merely runs."""
    from sdformerflow_amd.spikingjelly_compat import functional
    from test_train_gpu import small_model
    lr, wd, clip = 1e-3, 0.01, 100.0
    model, chunk, label, mask = small_model()
    twin = small_model()[0]
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    names = {p: n for n, p in model.named_parameters()}

    topt = torch.optim.AdamW(twin.parameters(), lr=lr, weight_decay=wd, foreach=False)
    ts = torch.amp.GradScaler("cuda", init_scale=init_scale)
    twin.train()
    functional.reset_net(twin)
    with torch.autocast("cuda", dtype=torch.float16):
        flows = train.forward_train(twin, chunk)
    t_loss = train.flow_loss_supervised([f.float() for f in flows], label, mask, 1.0, 1.0, n_valid=train.global_valid_count(mask))
    ts.scale(t_loss).backward()
    torch.nn.utils.clip_grad_norm_([p for p in twin.parameters() if p.grad is not None], clip)
    ts.step(topt)
    ts.update()
    tparams = dict(twin.named_parameters())
    t_skipped = all(torch.equal(p, start[n]) for n, p in tparams.items())

    buckets = train.GradientBuckets(model.parameters())
    opt = train.BucketAdamW(buckets, lr, weight_decay=wd)
    scaler = train.LossScaler(init_scale=init_scale, device=DEV)
    records = []
    with hip.launch_log() as log:
        loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=clip, amp="fp16", scaler=scaler, grads_out=records)
    kernels = [kname(r[0]) for r in log.rows]
    nb = len(buckets.flat)
    assert kernels[-(3 * nb + 1):] == ["grad_stats_partial_kernel", "grad_stats_finish_kernel"] * nb + ["grad_clip_scale_coef_kernel"] + ["adamw_step_scaled_kernel"] * nb
    st = hip.loss_scale_read(scaler.state)
    _, (total, bad), coef = opt.stats.read()
    skipped = bool(st["found_inf"])
    print(f"init_scale {init_scale}: loss {float(loss)!r} (twin {float(t_loss)!r}), scaled norm {total!r}, non-finite {bad}, coef {coef!r}, "
          f"skipped {skipped} (twin {t_skipped}), scale afterwards {st['scale']} (twin {ts.get_scale()})")
    assert torch.isfinite(loss) and skipped == t_skipped and st["scale"] == ts.get_scale() and st["growth_tracker"] == int(ts._growth_tracker)
    assert len(records) == 1 and scaler.skipped == int(skipped)
    if skipped:
        assert all(torch.equal(p, start[n]) for n, p in model.named_parameters())
        assert all(float(opt.state[p]["step"]) == 0.0 and not opt.state[p]["exp_avg"].any() for p in buckets.params)
    else:
        d, errs = 0.0, {}
        for p in buckets.params:
            n = names[p]
            if p.grad is None:
                assert tparams[n].grad is None and torch.equal(p, start[n])
                continue
            zeros = np.zeros(p.numel())
            want = train.adamw_restatement(np64(start[n]), np64(buckets._views[p]) * st["inv_scale"], zeros, zeros, 1, lr, BETAS, EPS, wd, coef)[0]
            t_want = train.adamw_restatement(np64(start[n]), np64(tparams[n].grad), zeros, zeros, 1, lr, BETAS, EPS, wd)[0]      # (clipped and unscaled in place)
            d = max(d, float(np.abs(np64(tparams[n]) - t_want).max()))
            errs[n] = (np.abs(np64(p) - want), ulp32(want))
        print(f"torch's distance from the fp64 restatement d {d:.3e}; the kernel's {max(float(e.max()) for e, _ in errs.values()):.3e}")
        for n, (err, ulp) in errs.items():
            assert (err <= np.maximum(2.0 * d, ulp)).all(), (n, float(err.max()), d)
        true_units = train.get_grads(model, buckets, unscale=True, scaler=scaler)
        k = next(iter(records[0]))
        assert abs(true_units[k] - records[0][k] * st["inv_scale"]) <= 1e-12 * abs(true_units[k])
    # a second step merely runs
    train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=clip, amp="fp16", scaler=scaler, grads_out=records)
    assert len(records) == 2 and all(torch.isfinite(p).all() for p in buckets.params) and scaler.skipped in (int(skipped), int(skipped) + 1)
