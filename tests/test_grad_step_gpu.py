"""The training step's HIP tail on the GPU (csrc/grad_step.hip): the statistics kernel bit for bit / to the fp64 summation bound on
segments packed off every alignment, the clip coefficient to one fp32 rounding, the AdamW kernel against the fp64 restatement
within twice torch's own fp32 distance from it, and one whole train_step with train.BucketAdamW beside a twin stepped by
clip_grad_norm_ + torch.optim.AdamW."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import hip, train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 4095, 4096, 4097, 70001)     # back to back: most start off a 16-byte boundary
OFFSETS = tuple(int(v) for v in np.cumsum((0,) + LENGTHS[:-1]))
TOTAL = sum(LENGTHS)
NONFINITE_SEG = 9                                                       # the 4095-float segment carries inf, -inf and NaN
GUARD = 0x5A
U53 = 2.0 ** -53


def kname(logged):
    """`grad_stats_partial_kernel` of the launch log's `(anonymous namespace)::grad_stats_partial_kernel(float const*, ...)`."""
    m = re.search(r"(\w+)(?:<.*?>)?\(", logged)
    return m.group(1) if m else logged


def make_values(seed):
    """Normal draws, with zeros, denormals and negative zeros sprinkled over every segment that has room, and the three
    non-finite values in one segment."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(TOTAL).astype(np.float32)
    for off, n in zip(OFFSETS, LENGTHS):
        if n >= 63:
            idx = off + rng.choice(n, size=9, replace=False)
            g[idx[0:3]] = 0.0
            g[idx[3:6]] = np.array([1e-42, -3e-45, 1.1e-38], dtype=np.float32)
            g[idx[6:9]] = -0.0
    g[OFFSETS[4]] = -0.0                                                 # ... and in a short one
    bad = OFFSETS[NONFINITE_SEG] + np.array([0, 1234, 4094])
    g[bad] = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
    return g


def guarded(nbytes, align=256):
    """(outer uint8 tensor filled with the guard byte, offset of an `align`-aligned window of nbytes with >= 256 guard bytes each side)."""
    outer = torch.full((nbytes + 3 * align + 512,), GUARD, dtype=torch.uint8, device=DEV)
    off = 256 + (-(outer.data_ptr() + 256)) % align
    return outer, off


def guards_intact(outer, off, nbytes):
    return bool((outer[:off] == GUARD).all()) and bool((outer[off + nbytes:] == GUARD).all())


def carve(outer, off, dtype, n):
    return outer[off:off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype)


def run_stats(flat, seg):
    """sdf_grad_stats_fwd called directly: the table and the workspace are windows between guard bytes.  Returns the table (numpy)."""
    lib = hip.lib()
    ws_bytes = lib.sdf_grad_stats_workspace_bytes(seg.n)
    t_outer, t_off = guarded(seg.n * 40)
    w_outer, w_off = guarded(ws_bytes)
    d = hip.GradStatsDesc()
    d.flat, d.n, d.seg_host, d.seg, d.nseg = flat.data_ptr(), flat.numel(), seg.host.ctypes.data, seg.dev.data_ptr(), seg.n
    d.row0, d.rows, d.table, d.workspace, d.workspace_bytes = 0, seg.n, t_outer.data_ptr() + t_off, w_outer.data_ptr() + w_off, ws_bytes
    assert lib.sdf_grad_stats_fwd(C.byref(d), hip._stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(t_outer, t_off, seg.n * 40) and guards_intact(w_outer, w_off, ws_bytes)
    return carve(t_outer, t_off, torch.float64, seg.n * 5).view(seg.n, 5).cpu().numpy().copy()


@pytest.fixture(scope="module")
def values():
    g = make_values(7)
    _, rows = train.grad_stats_record({i: g[o:o + n] for i, (o, n) in enumerate(zip(OFFSETS, LENGTHS))})
    return g, rows


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_grad_stats_on_packed_segments(values, shift):
    """The whole buffer carved at element offset `shift` of an aligned allocation.  min_abs, max_abs and nonfinite bit for bit; sum_abs and
    sum_sq within (n - 1) 2^-53 relative of math.fsum of the same fp64 terms (all non-negative: the bound of any summation order); a
    second run gives the same bytes."""
    g, rows = values
    outer = torch.zeros(TOTAL + 8, dtype=torch.float32, device=DEV)
    flat = outer[shift:shift + TOTAL]
    flat.copy_(torch.from_numpy(g))
    assert flat.data_ptr() % 16 == 4 * shift
    seg = hip.GradSegments(zip(OFFSETS, LENGTHS), DEV)
    with hip.launch_log() as log:
        got = run_stats(flat, seg)
    assert [kname(r[0]) for r in log.rows] == ["grad_stats_partial_kernel", "grad_stats_finish_kernel"], log.rows
    assert [(r[1], r[2]) for r in log.rows] == [(128 * len(LENGTHS), 256), (len(LENGTHS), 64)]
    for s, n in enumerate(LENGTHS):
        sum_abs, sum_sq, mn, mx, bad = rows[s]
        print(f"segment {s} (n {n}): sum_abs {got[s, 0]!r} vs fsum {sum_abs!r}, sum_sq {got[s, 1]!r} vs {sum_sq!r}, bound {(n - 1) * U53:.2e}")
        assert got[s, 2:].tobytes() == np.array([mn, mx, bad]).tobytes(), (s, got[s], rows[s])
        assert abs(got[s, 0] - sum_abs) <= (n - 1) * U53 * sum_abs and abs(got[s, 1] - sum_sq) <= (n - 1) * U53 * sum_sq, (s, got[s], rows[s])
    assert got[NONFINITE_SEG, 4] == 3.0 and got[:, 4].sum() == 3.0 and got[4, 2] == 0.0
    assert run_stats(flat, seg).tobytes() == got.tobytes()
    # the wrapper: its own workspace, rows of a larger table, the others left alone
    table = torch.full((len(LENGTHS) + 3, 5), -7.0, dtype=torch.float64, device=DEV)
    assert hip.grad_stats(flat, seg, table, row=2) is table
    assert table[2:-1].cpu().numpy().tobytes() == got.tobytes() and bool((table[:2] == -7.0).all()) and bool((table[-1] == -7.0).all())


def test_grad_stats_of_a_segment_without_a_finite_element():
    flat = torch.tensor([float("nan"), float("inf"), 1.0, -2.0], device=DEV)
    got = hip.grad_stats(flat, [(0, 2), (2, 2)]).cpu().numpy()
    assert got[0].tolist() == [0.0, 0.0, math.inf, 0.0, 2.0] and got[1].tolist() == [3.0, 5.0, 1.0, 2.0, 0.0]


@pytest.mark.parametrize("case,scale,max_norm", [("above", 1.0, 100.0), ("below", 1e-3, 100.0), ("zero", 0.0, 100.0), ("tiny_norm", 1.0, 0.125)])
def test_clip_coefficient(case, scale, max_norm):
    """coef within one fp32 rounding (2^-23 relative) of the fp64 formula on the exact sums of squares; rows outside the mask do not
    count.  torch's own fp32 value is printed beside it."""
    g = make_values(3)
    g[~np.isfinite(g)] = 0.5
    g = (g * np.float32(scale)).astype(np.float32)
    flat = torch.from_numpy(g).to(DEV)
    seg = hip.GradSegments(zip(OFFSETS, LENGTHS), DEV)
    table = hip.grad_stats(flat, seg)
    _, rows = train.grad_stats_record({i: g[o:o + n] for i, (o, n) in enumerate(zip(OFFSETS, LENGTHS))})
    for mask in (None, [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0]):
        use = [r[1] for i, r in rows.items() if mask is None or mask[i]]
        want, total = train.clip_coef_restatement(use, max_norm)
        m = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=DEV)
        c_outer, c_off = guarded(4)
        r_outer, r_off = guarded(16)
        coef, record = hip.grad_clip_coef(table, max_norm, m, carve(c_outer, c_off, torch.float32, 1), carve(r_outer, r_off, torch.float64, 2))
        torch.cuda.synchronize()
        assert guards_intact(c_outer, c_off, 4) and guards_intact(r_outer, r_off, 16)
        parts = [flat[o:o + n] for i, (o, n) in enumerate(zip(OFFSETS, LENGTHS)) if mask is None or mask[i]]
        t_coef = float(torch.clamp(max_norm / (torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p) for p in parts])) + 1e-6), max=1.0))
        print(f"{case} mask {mask is not None}: total {float(record[0])!r} (fp64 {total!r}), coef {float(coef)!r}, fp64 formula {want!r}, torch fp32 {t_coef!r}")
        assert abs(float(coef) - want) <= 2.0 ** -23 * want and abs(float(record[0]) - total) <= len(use) * U53 * total
        assert float(record[1]) == 0.0 and (float(coef) == 1.0) == (case in ("below", "zero"))
    # no clip: max_norm inf gives exactly 1, and the non-finite count of the statistics arrives in the record
    table[5, 4] = 2.0
    coef, record = hip.grad_clip_coef(table, float("inf"))
    assert float(coef) == 1.0 and float(record[1]) == 2.0


# ------------------------------------------------------------------------------------------------ AdamW
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
INACTIVE = 6                                                            # the 64-float segment gets no update


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def torch_adamw_cpu(p, g, m, v, step0, wd, coef):
    """torch.optim.AdamW(foreach=False) on CPU fp32 tensors, one step from the state (m, v, step0), the gradient multiplied by the fp32
    coefficient first, as clip_grad_norm_ does."""
    ps = [torch.nn.Parameter(torch.from_numpy(p[o:o + n].copy())) for o, n in zip(OFFSETS, LENGTHS)]
    opt = torch.optim.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    for i, (q, o, n) in enumerate(zip(ps, OFFSETS, LENGTHS)):
        if i == INACTIVE:
            continue
        q.grad = torch.from_numpy(g[o:o + n].copy()).mul_(torch.tensor(coef, dtype=torch.float32))
        opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(m[o:o + n].copy()),
                        "exp_avg_sq": torch.from_numpy(v[o:o + n].copy())}
    opt.step()
    out = [a.copy() for a in (p, m, v)]
    for i, (q, o, n) in enumerate(zip(ps, OFFSETS, LENGTHS)):
        if i != INACTIVE:
            out[0][o:o + n], out[1][o:o + n], out[2][o:o + n] = q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()
    return out


@pytest.mark.parametrize("layout", ["mirror", "own"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_kernel(layout, wd, clip):
    """Steps 1, 2, 3 from zero moments and one step from a state preloaded to step 1000.  `mirror`: the parameters are packed like the
    bucket (16 bytes per lane on every stream); `own`: every parameter starts on its own 16-byte boundary, as separate allocations do
    (the parameter stream is then read 4 bytes per lane wherever its segment starts elsewhere).  d = the largest elementwise distance of
    torch's fp32 AdamW(foreach=False) on the CPU from the fp64 restatement, on the same inputs; the kernel may be 2 d from the
    restatement, or one ulp of the value where that is more."""
    rng = np.random.default_rng(100 + 2 * int(clip) + int(wd > 0))
    coef = np.float32(0.3712) if clip else np.float32(1.0)
    p_offs = OFFSETS if layout == "mirror" else tuple(int(v) for v in np.cumsum([0] + [(n + 3) // 4 * 4 + 4 for n in LENGTHS[:-1]]))
    p_total = p_offs[-1] + LENGTHS[-1]
    shift = 1                                                            # the three flat buffers sit one float off a 16-byte boundary
    outers = {k: guarded((TOTAL + shift) * 4) for k in "gmv"}
    p_shift = shift if layout == "mirror" else 0                        # mirror: the parameters share the buckets' position too
    outers["p"] = guarded((p_total + p_shift) * 4)
    flat = {k: carve(o, off, torch.float32, TOTAL + shift)[shift:] for k, (o, off) in outers.items() if k != "p"}
    pbuf = carve(*outers["p"], torch.float32, p_total + p_shift)[p_shift:]
    pad = torch.ones(p_total, dtype=torch.bool)
    for o, n in zip(p_offs, LENGTHS):
        pad[o:o + n] = False
    pad_bytes = pbuf.view(torch.uint8).view(-1, 4)[pad.to(DEV)].clone()

    def get_p():
        host = pbuf.cpu().numpy()
        return np.concatenate([host[o:o + n] for o, n in zip(p_offs, LENGTHS)])

    def put(buf, arr):
        buf.copy_(torch.from_numpy(arr))

    p = rng.standard_normal(TOTAL).astype(np.float32)
    p[rng.choice(TOTAL, 50, replace=False)] = 0.0
    m, v = np.zeros(TOTAL, np.float32), np.zeros(TOTAL, np.float32)
    for o, po, n in zip(OFFSETS, p_offs, LENGTHS):
        pbuf[po:po + n] = torch.from_numpy(p[o:o + n]).to(DEV)
    put(flat["m"], m)
    put(flat["v"], v)
    coef_dev = torch.tensor([float(coef)], dtype=torch.float32, device=DEV)
    rows = hip.adamw_rows(len(LENGTHS))
    rows["offset"], rows["length"], rows["active"] = OFFSETS, LENGTHS, 1
    rows["active"][INACTIVE] = 0
    rows["param"] = [pbuf.data_ptr() + 4 * po for po in p_offs]
    worst = {}
    for step in (1, 2, 3, 1001):
        if step == 1001:                                                 # a long-trained state
            m = (0.1 * rng.standard_normal(TOTAL)).astype(np.float32)
            v = (0.01 * rng.random(TOTAL)).astype(np.float32)
            put(flat["m"], m)
            put(flat["v"], v)
        g = make_values(step)
        g[~np.isfinite(g)] = 0.0
        put(flat["g"], g)
        for name, val in zip(("decay", "w1", "beta2", "w2", "neg_step_size", "bc2_sqrt", "eps"), train.adamw_scalars(step, LR, BETAS, EPS, wd)):
            rows[name] = val
        with hip.launch_log() as log:
            hip.adamw_step(flat["g"], flat["m"], flat["v"], rows, None, coef_dev if clip else None)
        torch.cuda.synchronize()
        assert [(kname(r[0]), r[1], r[2]) for r in log.rows] == [("adamw_step_kernel", 128 * len(LENGTHS), 256)]
        got = get_p(), flat["m"].cpu().numpy(), flat["v"].cpu().numpy()
        want = [np.concatenate(x) for x in zip(*[train.adamw_restatement(p[o:o + n], g[o:o + n], m[o:o + n], v[o:o + n], step, LR, BETAS, EPS, wd, float(coef))
                                                 if i != INACTIVE else (p[o:o + n].astype(np.float64), m[o:o + n].astype(np.float64), v[o:o + n].astype(np.float64))
                                                 for i, (o, n) in enumerate(zip(OFFSETS, LENGTHS))])]
        ref = torch_adamw_cpu(p, g, m, v, step - 1, wd, float(coef))
        for name, a, w, r in zip("pmv", got, want, ref):
            d = float(np.abs(r.astype(np.float64) - w).max())
            err = np.abs(a.astype(np.float64) - w)
            worst[name] = max(worst.get(name, (0.0, 0.0)), (float(err.max()), d))
            print(f"{layout} wd {wd} clip {clip} step {step} {name}: torch d {d:.3e}, kernel {err.max():.3e}, differs from torch in {int((a != r).sum())} of {a.size}")
            assert (err <= np.maximum(2.0 * d, ulp32(w))).all(), (name, step, float(err.max()), d)
        o, n = OFFSETS[INACTIVE], LENGTHS[INACTIVE]
        assert all(a[o:o + n].tobytes() == b[o:o + n].tobytes() for a, b in zip(got, (p, m, v)))        # not touched, bit for bit
        assert flat["g"].cpu().numpy().tobytes() == g.tobytes()                                            # the gradient is only read
        p, m, v = got
    assert all(guards_intact(o, off, (TOTAL + shift) * 4) for k, (o, off) in outers.items() if k != "p")
    assert guards_intact(*outers["p"], (p_total + p_shift) * 4) and torch.equal(pbuf.view(torch.uint8).view(-1, 4)[pad.to(DEV)], pad_bytes)
    for k, (o, off) in outers.items():                                   # ... and the float in front of each shifted buffer
        assert bool((o[off:off + 4 * (p_shift if k == "p" else shift)] == GUARD).all())


def test_bucket_adamw_leaves_a_parameter_without_gradient_alone():
    """BucketAdamW over parameters of the packed lengths, one of them without a gradient: its value, moments and step count stay, the
    others advance; every updated parameter's version counter moves; the clip record holds the norm."""
    torch.manual_seed(4)
    params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in reversed(LENGTHS)]        # (buckets fill in reverse order)
    buckets = train.GradientBuckets(params)
    assert [p.numel() for p in buckets.buckets[0]] == list(LENGTHS)
    opt = train.BucketAdamW(buckets, LR, weight_decay=0.01)
    skip = params[3]
    for step in (1, 2):
        buckets.begin()
        for p in params:
            p.grad.copy_(torch.randn_like(p))
        skip.grad = None
        before = {p: (p.detach().clone(), p._version) for p in params}
        norm = torch.linalg.vector_norm(torch.cat([p.grad for p in params if p.grad is not None]).double()).item()
        opt.step(1.0)
        _, (total, bad), coef = opt.stats.read()
        assert abs(total - norm) <= 1e-12 * norm and bad == 0.0 and abs(coef - 1.0 / (norm + 1e-6)) <= 2.0 ** -23 * coef
        for p in params:
            st = opt.state[p]
            if p is skip:
                assert torch.equal(p, before[p][0]) and p._version == before[p][1] and float(st["step"]) == 0.0
                assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
            else:
                assert not torch.equal(p, before[p][0]) and p._version > before[p][1] and float(st["step"]) == float(step)
                assert torch.isfinite(p).all() and st["exp_avg"].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ one whole step
@pytest.fixture
def deterministic_convolutions():
    """The library's convolution weight gradients add with float atomics by default: two backward passes of the same weights and inputs
    then differ in the last bits of 9 of this model's 225 gradients (measured: up to 9e-7 of a tensor's largest element), and the
    smallest |g| of a tensor - a cancelling sum - by more than the 1e-6 the record is held to.  With the deterministic algorithms the
    two passes are bit-equal, and the twin's gradients ARE the model's."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def test_train_step_with_bucket_adamw_beside_a_torch_twin(deterministic_convolutions):
    """One train_step of the smallest model test_train_gpu.py trains, with BucketAdamW, beside a twin from the same weights and inputs
    stepped by clip_grad_norm_ + torch.optim.AdamW, with a clip_grad below the measured norm.  Only this ONE step is compared value
    for value (from the second on, ulp differences in the weights may flip spikes); a second step must merely run."""
    from test_train_gpu import CFG, small_kwargs, small_model
    lr, wd = 1e-3, 0.01
    model, chunk, label, mask = small_model()
    twin = small_model()[0]
    names = {p: n for n, p in model.named_parameters()}
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()))

    # the twin: the parent's tail.  Its norm is measured first, so that the clip acts (clip_grad below the norm)
    # (by a step that changes no parameter - SGD at lr 0; it moves only BatchNorm's running statistics, which a train-mode step does not read)
    tb = train.GradientBuckets(twin.parameters())
    train.train_step(twin, torch.optim.SGD(twin.parameters(), lr=0.0), chunk, label, mask, buckets=tb, clip_grad=None)
    assert all(torch.equal(p, start[n]) for n, p in twin.named_parameters())
    norm = float(torch.linalg.vector_norm(torch.cat([f.double() for f in tb.flat])))
    clip_grad = float(np.float32(0.5 * norm))
    topt = torch.optim.AdamW(twin.parameters(), lr=lr, weight_decay=wd)
    t_rec = []
    train.train_step(twin, topt, chunk, label, mask, buckets=tb, clip_grad=clip_grad, grads_out=t_rec)

    model.eval()                                                         # a packed inference plan of the OLD weights exists
    with torch.no_grad():
        before = [f.clone() for f in model(chunk)["flow"]]
    e0 = model.engine()
    buckets = train.GradientBuckets(model.parameters())
    opt = train.BucketAdamW(buckets, lr, weight_decay=wd)
    versions = {p: p._version for p in model.parameters()}
    records = []
    with hip.launch_log() as log:
        loss = train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=clip_grad, grads_out=records)
    kernels = [kname(r[0]) for r in log.rows]
    nb = len(buckets.flat)
    assert kernels[-(3 * nb + 1):] == ["grad_stats_partial_kernel", "grad_stats_finish_kernel"] * nb + ["grad_clip_coef_kernel"] + ["adamw_step_kernel"] * nb
    assert torch.isfinite(loss)
    _, (total, bad), coef = opt.stats.read()
    print(f"norm {total!r} (probe {norm!r}), clip_grad {clip_grad!r}, coef {coef!r}")
    assert bad == 0.0 and coef < 1.0 and abs(coef - clip_grad / (total + 1e-6)) <= 2.0 ** -23 * coef

    # every parameter: the kernel's distance from the fp64 restatement of ITS gradients (the buckets still hold them, unscaled) within
    # twice the distance of torch's own result - the twin's - from the restatement of the twin's, with a floor of one ulp
    tparams = dict(twin.named_parameters())
    no_grad, d, worst, twin_equal = [], 0.0, 0.0, 0
    errs = {}
    for p in buckets.params:
        n = names[p]
        if p.grad is None:
            no_grad.append(n)
            assert torch.equal(p, start[n]) and p._version == versions[p] and float(opt.state[p]["step"]) == 0.0
            assert tparams[n].grad is None and torch.equal(tparams[n], start[n])
            continue
        assert p._version > versions[p], n
        zeros = np.zeros(p.numel())
        want = train.adamw_restatement(start[n].cpu().numpy().ravel(), buckets._views[p].cpu().numpy().ravel(), zeros, zeros, 1, lr, BETAS, EPS, wd, coef)[0]
        # (the twin's gradients were clipped in place: its restatement takes them as they are)
        t_want = train.adamw_restatement(start[n].cpu().numpy().ravel(), tparams[n].grad.cpu().numpy().ravel(), zeros, zeros, 1, lr, BETAS, EPS, wd)[0]
        d = max(d, float(np.abs(tparams[n].detach().cpu().numpy().ravel().astype(np.float64) - t_want).max()))
        errs[n] = (np.abs(p.detach().cpu().numpy().ravel().astype(np.float64) - want), ulp32(want))
        worst = max(worst, float(errs[n][0].max()))
        twin_equal += int(torch.equal(p, tparams[n]))
    print(f"torch's distance from the fp64 restatement d {d:.3e}; the kernel's {worst:.3e}; {twin_equal} of {len(errs)} parameters bit-equal to the twin's; "
          f"{len(no_grad)} without a gradient")
    for n, (err, ulp) in errs.items():
        assert (err <= np.maximum(2.0 * d, ulp)).all(), (n, float(err.max()), d)
    # (at this size every parameter receives a gradient; the `.grad = None` path: test_bucket_adamw_leaves_a_parameter_without_gradient_alone)

    # the stored record: the reference's keys, the clipped |grad| of the twin to 1e-6 relative
    assert len(records) == 1 and len(t_rec) == 1
    rec = records[0]
    want_keys = [f"{n}_{k}" for n, p in model.named_parameters() if p.requires_grad and "weight" in n and p.grad is not None for k in ("mean", "min", "max")]
    assert list(rec) == want_keys and list(t_rec[0]) == want_keys
    if any("weight" in n for n in no_grad):                              # the reference's get_grads stops at such a parameter
        with pytest.raises(AttributeError):
            train.get_grads(model, buckets, missing="raise")
    else:
        assert train.get_grads(model, buckets, missing="raise") == rec
    for n, tp in tparams.items():
        if "weight" in n and tp.grad is not None:
            a = tp.grad.abs().double()
            for k, w in (("mean", a.mean().item()), ("min", a.min().item()), ("max", a.max().item())):
                assert abs(rec[f"{n}_{k}"] - w) <= 1e-6 * w, (n, k, rec[f"{n}_{k}"], w)
                assert abs(t_rec[0][f"{n}_{k}"] - w) <= 1e-6 * w, (n, k)

    # the packed inference plan was rebuilt from the stepped weights
    model.eval()
    with torch.no_grad():
        after = [f.clone() for f in model(chunk)["flow"]]
    fresh = type(model)(*small_kwargs(yaml.safe_load(open(CFG))))
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh(chunk)["flow"]
    assert all(torch.equal(a, b) for a, b in zip(after, want))
    assert model.engine() is not e0 and not any(torch.equal(a, b) for a, b in zip(before, after))

    # a second step merely runs: finite parameters, step counts advanced
    train.train_step(model, opt, chunk, label, mask, buckets=buckets, clip_grad=clip_grad, grads_out=records)
    assert len(records) == 2 and list(records[1]) == want_keys
    for p in buckets.params:
        assert torch.isfinite(p).all() and float(opt.state[p]["step"]) == (0.0 if names[p] in no_grad else 2.0)


def test_save_grads_csv_of_device_records(tmp_path):
    import csv
    lin = torch.nn.Linear(6, 3).to(DEV)
    buckets = train.GradientBuckets(lin.parameters())
    path = str(tmp_path / "grads_w.csv")
    recs = []
    for k in range(2):
        buckets.begin()
        lin(torch.randn(4, 6, device=DEV)).square().sum().backward()
        buckets.finish()
        recs.append(train.get_grads(lin, buckets))
        train.save_grads_csv(recs[-1:], path)
    rows = list(csv.reader(open(path, newline="")))
    assert rows[0] == ["", "weight_mean", "weight_min", "weight_max"] and len(rows) == 3 and sum(r[0] == "" for r in rows) == 1
    for r, rec in zip(rows[1:], recs):
        assert [float(x) for x in r[1:]] == list(rec.values())
    assert abs(recs[1]["weight_max"] - lin.weight.grad.abs().max().item()) == 0.0
