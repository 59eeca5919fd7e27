"""Host side of the training step's HIP tail (csrc/grad_step.hip), no GPU: the numpy restatements of the three kernels against torch's
own clip_grad_norm_ / AdamW(foreach=False) / p.grad.abs() on CPU tensors and against the reference's get_grads record (fixture
golden/grad_stats.npz, made by golden/make_golden_grad_stats.py); the new entry points in the header, the binding and the build list;
every argument refusal, reported by the library before any launch; BucketAdamW's state interchange with torch.optim.AdamW; the CSV."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "grad_stats.npz"))
NEW = ("sdf_grad_stats_workspace_bytes", "sdf_grad_stats_fwd", "sdf_grad_clip_coef", "sdf_adamw_step")
U24 = 2.0 ** -24                       # one fp32 rounding
DENORM = 2.0 ** -149                   # the fp32 grid below 2^-126


def loaded_lib():
    from sdformerflow_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.lib()


# ------------------------------------------------------------------------------------------------ restatements
def test_statistics_restatement_matches_the_reference_record():
    """train.grad_stats_record on the fixture's gradients against what the reference's get_grads recorded from them.  The reference
    works in fp32: its min and max are exact, its mean is an fp32 sum of n values ((n - 1) roundings at the most) and a division."""
    from sdformerflow_amd import train
    names = [str(n) for n in G["names"]]
    grads = {n: G["grad/" + n] for n in names if "weight" in n}
    rec, rows = train.grad_stats_record(grads)
    assert list(rec) == [str(k) for k in G["keys"]]                          # the reference's keys, in its order; no bias
    for k, want in zip(G["keys"], G["values"]):
        k = str(k)
        n = grads[k.rsplit("_", 1)[0]].size
        tol = (n * U24 * abs(want) + DENORM) if k.endswith("_mean") else 0.0
        assert abs(rec[k] - want) <= tol, (k, rec[k], want)
    # after the clip: the reference multiplied every gradient by the fp32 coefficient (one more rounding per element)
    coef, total = train.clip_coef_restatement([r[1] for r in train.grad_stats_record({n: G["grad/" + n] for n in names})[1].values()], 0.5)
    assert abs(total - float(G["clip_total"])) <= len(names) * 64 * U24 * total          # torch: fp32 norms of fp32 norms
    rec_c, _ = train.grad_stats_record(grads, coef)
    for k, want in zip(G["clip_keys"], G["clip_values"]):
        k = str(k)
        n = grads[k.rsplit("_", 1)[0]].size
        assert abs(rec_c[k] - want) <= (n + 64) * U24 * abs(want) + DENORM, (k, rec_c[k], want)


def test_statistics_restatement_matches_torch_and_handles_nonfinite():
    from sdformerflow_amd import train
    g = torch.randn(3, 37, generator=torch.Generator().manual_seed(5))
    g[1, 4], g[2, 0] = 0.0, -0.0
    rec, rows = train.grad_stats_record({"a.weight": g.numpy()})
    assert rec["a.weight_min"] == g.abs().min().item() == 0.0 and rec["a.weight_max"] == g.abs().max().item()
    assert abs(rec["a.weight_mean"] - g.abs().mean().item()) <= g.numel() * U24 * rec["a.weight_mean"]
    assert rows["a.weight"][1] == math.fsum(float(x) * float(x) for x in g.flatten().tolist()) and rows["a.weight"][4] == 0.0
    g[0, 0], g[0, 1], g[2, 5] = float("inf"), float("-inf"), float("nan")
    rec, rows = train.grad_stats_record({"a.weight": g.numpy()})
    assert all(math.isnan(rec[k]) for k in rec) and rows["a.weight"][4] == 3.0
    fin = g.flatten()[torch.isfinite(g.flatten())].double()
    assert rows["a.weight"][0] == math.fsum(fin.abs().tolist()) and rows["a.weight"][3] == fin.abs().max().item()
    _, rows = train.grad_stats_record({"e": np.array([np.nan], dtype=np.float32)})
    assert rows["e"] == (0.0, 0.0, math.inf, 0.0, 1.0)                       # nothing finite: the identities


@pytest.mark.parametrize("scale,max_norm", [(10.0, 1.0), (0.01, 1.0), (0.0, 1.0), (1.0, 100.0)])
def test_clip_restatement_matches_clip_grad_norm(scale, max_norm):
    from sdformerflow_amd import train
    gen = torch.Generator().manual_seed(11)
    ps = [torch.nn.Parameter(torch.zeros(s)) for s in ((7, 5), (13,), (1,), (4, 3, 3))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen) * scale
    _, rows = train.grad_stats_record({str(i): p.grad.numpy() for i, p in enumerate(ps)})
    coef, total = train.clip_coef_restatement([r[1] for r in rows.values()], max_norm)
    before = [p.grad.clone() for p in ps]
    t_total = torch.nn.utils.clip_grad_norm_(ps, max_norm).item()
    assert abs(total - t_total) <= 64 * U24 * total
    assert (coef == 1.0) == (total + 1e-6 <= max_norm)
    for p, b in zip(ps, before):                                          # what torch multiplied by is our coefficient, to fp32 rounding
        assert torch.allclose(p.grad.double(), b.double() * coef, rtol=64 * U24, atol=0.0)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adamw_restatement_matches_torch(wd):
    """train.adamw_restatement (fp64) chained over three steps against torch.optim.AdamW(foreach=False) in fp64 - the same arithmetic
    in another order: agreement to a few fp64 roundings - and in fp32: to a few fp32 roundings of the parameter."""
    from sdformerflow_amd import train
    gen = torch.Generator().manual_seed(3)
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-6)):
        p = torch.nn.Parameter(torch.randn(257, generator=gen).to(dtype))
        opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
        rp, rm, rv = p.detach().double().numpy().copy(), np.zeros(257), np.zeros(257)
        for step in (1, 2, 3):
            g = torch.randn(257, generator=gen).to(dtype)
            p.grad = g.clone()
            opt.step()
            rp, rm, rv = train.adamw_restatement(rp, g.double().numpy(), rm, rv, step, 1e-3, (0.9, 0.999), 1e-8, wd)
            assert np.abs(p.detach().double().numpy() - rp).max() <= tol * np.abs(rp).max()
            assert np.abs(opt.state[p]["exp_avg"].double().numpy() - rm).max() <= tol * np.abs(rm).max()
            assert np.abs(opt.state[p]["exp_avg_sq"].double().numpy() - rv).max() <= tol * np.abs(rv).max()
    # the clip coefficient multiplies the gradient
    a = train.adamw_restatement(rp, 0.25 * g.double().numpy(), rm, rv, 4, 1e-3)
    b = train.adamw_restatement(rp, g.double().numpy(), rm, rv, 4, 1e-3, coef=0.25)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_are_declared_bound_and_built():
    from sdformerflow_amd import hip
    hdr = open(os.path.join(ROOT, "include", "sdformerflow_hip.h")).read()
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, hdr, flags=re.M), name
        assert name in hip.SIGNATURES
    for s in ("SdfGradStatsDesc", "SdfAdamwRow", "SdfAdamwDesc"):
        assert "typedef struct %s" % s in hdr
    assert hip.SIGNATURES["sdf_grad_stats_fwd"] == (C.c_int, (C.POINTER(hip.GradStatsDesc), C.c_void_p))
    assert hip.SIGNATURES["sdf_adamw_step"] == (C.c_int, (C.POINTER(hip.AdamwDesc), C.c_void_p))
    assert hip.adamw_rows(3).dtype.itemsize == C.sizeof(hip.AdamwRow) == 56
    assert int(re.search(r"#define\s+SDF_VERSION\s+(\d+)", hdr).group(1)) == 107         # (additive exports: the version stays)
    assert " grad_step " in open(os.path.join(ROOT, "sdformerflow_amd", "csrc", "build.sh")).read()
    lib = loaded_lib()
    assert all(hasattr(lib, n) for n in NEW) and lib.sdf_version() == 107


P = 0x10000                             # a dummy pointer: every refusal below comes before anything dereferences it on the device


def stats_rc(lib, pairs=((0, 5), (5, 1), (6, 100)), **kw):
    from sdformerflow_amd import hip
    seg = np.ascontiguousarray(np.array(pairs, dtype=np.int64).reshape(-1, 2))
    d = hip.GradStatsDesc()
    d.flat = d.seg = d.table = d.workspace = P
    d.seg_host, d.n, d.nseg, d.row0, d.rows, d.workspace_bytes = seg.ctypes.data, 106, len(seg), 0, len(seg), 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.sdf_grad_stats_fwd(C.byref(d), None)


def test_grad_stats_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()
    assert lib.sdf_grad_stats_workspace_bytes(3) == 3 * 128 * 5 * 8                 # 128 partial records of 5 doubles per segment
    assert lib.sdf_grad_stats_workspace_bytes(0) == 0 and lib.sdf_grad_stats_workspace_bytes(65536) == 0
    assert lib.sdf_grad_stats_fwd(None, None) == hip.E_NULL
    for f in ("flat", "seg_host", "seg", "table", "workspace"):
        assert stats_rc(lib, **{f: None}) == hip.E_NULL, f
    assert stats_rc(lib, nseg=0) == hip.E_SHAPE and stats_rc(lib, n=0) == hip.E_SHAPE            # zero segments, an empty buffer
    assert stats_rc(lib, pairs=((-1, 5), (5, 1))) == hip.E_SHAPE                                 # a negative offset
    assert stats_rc(lib, pairs=((0, 5), (4, 3))) == hip.E_SHAPE                                  # overlapping
    assert stats_rc(lib, pairs=((5, 1), (0, 5))) == hip.E_SHAPE                                  # not ascending
    assert stats_rc(lib, pairs=((0, 5), (5, 0))) == hip.E_SHAPE                                  # an empty segment
    assert stats_rc(lib, pairs=((0, 5), (6, 101))) == hip.E_SHAPE                                # past the buffer
    assert stats_rc(lib, pairs=((0, 5), ((1 << 62), (1 << 62)))) == hip.E_SHAPE                  # ... without overflowing on the way
    assert stats_rc(lib, row0=1) == hip.E_SHAPE and stats_rc(lib, row0=-1) == hip.E_SHAPE and stats_rc(lib, rows=2) == hip.E_SHAPE
    assert stats_rc(lib, workspace_bytes=3 * 128 * 40 - 1) == hip.E_SHAPE                        # a workspace that is too small
    assert stats_rc(lib, flat=P + 2) == hip.E_ALIGN and stats_rc(lib, table=P + 4) == hip.E_ALIGN
    assert stats_rc(lib, workspace=P + 4) == hip.E_ALIGN and stats_rc(lib, seg=P + 4) == hip.E_ALIGN
    assert stats_rc(lib, flat=P + 4) != hip.E_ALIGN                                              # any float boundary will do
    # host pointers: real, readable, correctly aligned host memory is refused all the same - nothing the runtime does not know as
    # device memory reaches a launch
    host = np.zeros(1 << 16, dtype=np.float64)
    h = host.ctypes.data
    assert stats_rc(lib, flat=h, seg=h, table=h, workspace=h, workspace_bytes=host.nbytes) == hip.E_DTYPE
    assert not host.any()


def test_grad_clip_coef_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()
    f = lambda table=P, rows=4, mask=None, max_norm=1.0, coef=P, record=P: lib.sdf_grad_clip_coef(table, rows, mask, max_norm, coef, record, None)
    assert f(table=None) == hip.E_NULL and f(coef=None) == hip.E_NULL and f(record=None) == hip.E_NULL
    assert f(rows=0) == hip.E_SHAPE and f(rows=(1 << 24) + 1) == hip.E_SHAPE
    assert f(max_norm=-1.0) == hip.E_SHAPE and f(max_norm=float("nan")) == hip.E_SHAPE
    assert f(table=P + 4) == hip.E_ALIGN and f(record=P + 4) == hip.E_ALIGN and f(coef=P + 2) == hip.E_ALIGN
    host = np.zeros(64, dtype=np.float64)
    h = host.ctypes.data
    assert f(table=h, coef=h, record=h + 8) == hip.E_DTYPE and f(table=h, coef=h, record=h + 8, max_norm=float("inf")) == hip.E_DTYPE
    assert not host.any()


def adamw_rc(lib, edit=None, **kw):
    from sdformerflow_amd import hip
    rows = hip.adamw_rows(3)
    rows["param"], rows["offset"], rows["length"], rows["active"] = P, (0, 5, 6), (5, 1, 100), 1
    if edit:
        edit(rows)
    d = hip.AdamwDesc()
    d.grad = d.exp_avg = d.exp_avg_sq = d.rows = P
    d.rows_host, d.n, d.nseg = rows.ctypes.data, 106, 3
    for k, v in kw.items():
        setattr(d, k, v)
    return lib.sdf_adamw_step(C.byref(d), None)


def test_adamw_step_refusals_come_before_any_launch():
    from sdformerflow_amd import hip
    lib = loaded_lib()

    def put(field, i, v):
        def edit(rows):
            rows[field][i] = v
        return edit
    assert lib.sdf_adamw_step(None, None) == hip.E_NULL
    for f in ("grad", "exp_avg", "exp_avg_sq", "rows_host", "rows"):
        assert adamw_rc(lib, **{f: None}) == hip.E_NULL, f
    assert adamw_rc(lib, put("param", 1, 0)) == hip.E_NULL                                   # an active row without its parameter
    assert adamw_rc(lib, lambda r: (put("param", 1, 0)(r), put("active", 1, 0)(r))) != hip.E_NULL      # ... an inactive one needs none
    assert adamw_rc(lib, nseg=0) == hip.E_SHAPE and adamw_rc(lib, nseg=65536) == hip.E_SHAPE
    assert adamw_rc(lib, put("offset", 0, -1)) == hip.E_SHAPE
    assert adamw_rc(lib, put("offset", 1, 4)) == hip.E_SHAPE                                 # overlaps its predecessor
    assert adamw_rc(lib, put("length", 1, 0)) == hip.E_SHAPE
    assert adamw_rc(lib, put("length", 2, 101)) == hip.E_SHAPE and adamw_rc(lib, n=105) == hip.E_SHAPE      # past the buffer
    assert adamw_rc(lib, grad=P + 2) == hip.E_ALIGN and adamw_rc(lib, rows=P + 4) == hip.E_ALIGN and adamw_rc(lib, coef=P + 2) == hip.E_ALIGN
    assert adamw_rc(lib, exp_avg=P + 4) == hip.E_ALIGN and adamw_rc(lib, exp_avg_sq=P + 8) == hip.E_ALIGN    # the moments mirror the bucket
    assert adamw_rc(lib, grad=P + 4, exp_avg=P + 20, exp_avg_sq=P + 36) != hip.E_ALIGN
    assert adamw_rc(lib, put("param", 2, P + 2)) == hip.E_ALIGN
    host = np.zeros(1 << 12, dtype=np.float32)
    h = host.ctypes.data
    assert adamw_rc(lib, lambda r: r["param"].fill(h), grad=h, exp_avg=h, exp_avg_sq=h, rows=h, coef=h) == hip.E_DTYPE
    assert not host.any()


def test_wrappers_refuse_cpu_tensors():
    from sdformerflow_amd import hip
    z = torch.zeros(16)
    with pytest.raises(hip.SdfError):
        hip.grad_stats(z, [(0, 16)])
    with pytest.raises(hip.SdfError):
        hip.grad_clip_coef(torch.zeros(2, 5, dtype=torch.float64), 1.0)
    rows = hip.adamw_rows(1)
    with pytest.raises(hip.SdfError):
        hip.adamw_step(z, z.clone(), z.clone(), rows)


# ------------------------------------------------------------------------------------------------ the optimiser's state, the CSV
def small_net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))


def test_bucket_adamw_state_interchanges_with_torch_adamw():
    from sdformerflow_amd import hip, train
    net = small_net()
    buckets = train.GradientBuckets(net.parameters(), bucket_bytes=200)      # two buckets
    opt = train.BucketAdamW(buckets, 2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.02)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1 and opt.param_groups[0]["params"] == buckets.params
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1], gamma=0.5)        # accepted as an optimiser; the lr is live
    assert opt.param_groups[0]["lr"] == 2e-3 and sched.get_last_lr() == [2e-3]
    views = {p: (opt.state[p]["exp_avg"].data_ptr(), opt.state[p]["exp_avg_sq"].data_ptr()) for p in buckets.params}
    flat_ptrs = [(m.data_ptr(), m.numel()) for m in opt.exp_avg]
    assert all(any(a <= ptr < a + 4 * n for a, n in flat_ptrs) for ptr, _ in views.values())        # the moments live in the flat buffers

    # ours -> torch: the hyper-parameters and an (empty) state arrive, and torch steps with them
    ref = torch.optim.AdamW(net.parameters(), lr=1.0)
    ref.load_state_dict(opt.state_dict())
    g = ref.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 0.02)
    net(torch.randn(2, 5)).sum().backward()
    ref.step()
    ref.step()

    # torch -> ours: copied INTO the flat views, which stay the state
    opt.load_state_dict(ref.state_dict())
    for p in buckets.params:
        st = opt.state[p]
        assert (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) == views[p]
        assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
        assert st["exp_avg"].abs().sum() > 0 and float(st["step"]) == 2.0 and st["step"] is not ref.state[p]["step"]
    for bi, b in enumerate(buckets.buckets):                                  # the flat buffers ARE the loaded moments, packed
        assert torch.equal(opt.exp_avg[bi], torch.cat([ref.state[p]["exp_avg"].flatten() for p in b]))
        assert torch.equal(opt.exp_avg_sq[bi], torch.cat([ref.state[p]["exp_avg_sq"].flatten() for p in b]))
    # ... and back again: the round trip is the identity
    ref2 = torch.optim.AdamW(net.parameters(), lr=1.0)
    ref2.load_state_dict(opt.state_dict())
    for p in buckets.params:
        assert all(torch.equal(ref2.state[p][k], ref.state[p][k]) for k in ("step", "exp_avg", "exp_avg_sq"))
    # a state that does not know a parameter (torch never stepped it): that one starts from zero
    sd = ref.state_dict()
    del sd["state"][0]
    opt.load_state_dict(sd)
    p0 = buckets.params[0]
    assert float(opt.state[p0]["step"]) == 0.0 and not opt.state[p0]["exp_avg"].any() and opt.state[p0]["exp_avg"].data_ptr() == views[p0][0]
    # no CPU fallback: the step is refused before anything is counted
    with pytest.raises(hip.SdfError):
        opt.step(1.0)
    assert float(opt.state[buckets.params[1]]["step"]) == 2.0


def test_train_step_refuses_what_it_cannot_serve():
    from sdformerflow_amd import train
    net = small_net()
    buckets = train.GradientBuckets(net.parameters())
    opt = train.BucketAdamW(buckets, 1e-3)
    with pytest.raises(ValueError, match="pass them as buckets="):
        train.train_step(net, opt, None, None, None)
    with pytest.raises(ValueError, match="pass buckets="):
        train.train_step(net, torch.optim.AdamW(net.parameters()), None, None, None, grads_out=[])
    with pytest.raises(TypeError):
        train.BucketAdamW(net.parameters(), 1e-3)
    with pytest.raises(ValueError):
        train.get_grads(net, buckets, missing="ignore")


def test_save_grads_csv_appends_without_a_second_header(tmp_path):
    import csv
    from sdformerflow_amd import train
    path = str(tmp_path / "grads_w.csv")
    recs = [{"a.weight_mean": 0.5, "a.weight_min": 0.0, "a.weight_max": 1e-42}, {"a.weight_mean": 0.25, "a.weight_min": float("nan"), "a.weight_max": 2.0}]
    train.save_grads_csv(recs[:1], path)
    train.save_grads_csv(recs, path)
    train.save_grads_csv([], path)
    rows = list(csv.reader(open(path, newline="")))
    assert rows[0] == ["", "a.weight_mean", "a.weight_min", "a.weight_max"] and len(rows) == 4
    assert [r[0] for r in rows[1:]] == ["0", "0", "1"]                                   # the index column of the reference's frames
    assert [float(v) for v in rows[1][1:]] == [0.5, 0.0, 1e-42] and float(rows[3][3]) == 2.0 and math.isnan(float(rows[3][2]))
    assert sum(r[0] == "" for r in rows) == 1
