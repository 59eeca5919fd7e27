"""The stand-alone neuron entry points launch the instantiation their T names, on the grid their size needs (csrc/host_launch.h:
sdf_dispatch over the T lists, sdf_quad_blocks).  For every launching entry point and every T of its list, at N = 1028 - two workgroups,
the second one ragged, the smallest size at which a wrong grid or a wrong instantiation shows (the gate: rows = 9, C = 96) - each
call goes through the C ABI and
  * runs under hip.launch_log(): the recorded kernels carry exactly that T (and PLIF / U8 / the vector width) in their template
    arguments, on the expected workgroups of 256 threads, followed by one finish launch where a reduction exists;
  * writes into a slice of a larger buffer, 64 guard elements on each side, NaN (fp32) or the byte 7 (spikes) everywhere
    beforehand: the guards hold the same bits afterwards and nothing of the fill is left where a result belongs;
  * runs twice: bit-equal, parameter gradients included.
No numeric tolerance: parity with the oracle stays with test_hip_kernels.py and the *_train_gpu.py suites, and every one of these
instantiations is compared by value with an fp64 autograd reference in test_neuron_parity_gpu.py (cases: neuron_train_cases.py)."""
import ctypes as C

import pytest
import torch

from sdformerflow_amd import hip
from sdformerflow_amd.synthetic import synth_uniform as rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, GUARD = 1028, 64
WGS = 2                                              # (1028 / 4 + 255) / 256
T_STREAM, T_GLIF, T_GATE = (1, 2, 4, 5, 8, 10, 16, 20), (2, 4, 5, 10, 20), (1, 2, 4)
ROWS, CC = 9, 96                                     # gate: 9 * 3 (row, head) pairs * 8 lanes = 216 lanes, one workgroup
GATE_WGS = 1
NAN_BITS = torch.tensor([float("nan")]).view(torch.int32).item()


def dev(t):
    return t.to(DEV).contiguous()


def f32(n):
    return torch.empty((n,), dtype=torch.float32, device=DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(call, n_out, expect, u8=False):
    """call(out pointer) -> (rc, [further result tensors]); n_out result elements; expect = [(kernel name part, workgroups)]."""
    runs = []
    for _ in range(2):
        buf = torch.full((GUARD + n_out + GUARD,), 7 if u8 else float("nan"), dtype=torch.uint8 if u8 else torch.float32, device=DEV)
        with hip.launch_log() as log:
            rc, extra = call(buf[GUARD:].data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert len(log.rows) == len(expect), log.rows
        for (name, wgs, threads, _, _), (part, want) in zip(log.rows, expect):
            assert part in name and wgs == want and threads == 256, (name, wgs, threads, part, want)
        bits = buf.cpu() if u8 else buf.cpu().view(torch.int32)
        fill = 7 if u8 else NAN_BITS
        assert bool((bits[:GUARD] == fill).all()) and bool((bits[GUARD + n_out:] == fill).all()), "a store outside the result"
        assert not bool((bits[GUARD:GUARD + n_out] == fill).any()) and not bool(torch.isnan(buf[GUARD:GUARD + n_out].float()).any())
        runs.append([bits] + [e.cpu().view(torch.int32) for e in extra])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two calls differ"


def xg(T, seed):
    return dev(rnd((T, N), seed, -0.3, 0.6)), dev(rnd((T, N), seed + 1, -1.0, 1.0))


def neuron_desc(x, out, T, kind=hip.SDF_LIF, u8=False, W=None, b=None):
    d = hip.NeuronDesc()
    d.x, d.out, d.T, d.out_dtype, d.kind = x.data_ptr(), out, T, hip.SDF_U8 if u8 else hip.SDF_F32, kind
    d.nb, d.ni, d.x_st, d.o_st = 1, N, N, N
    d.tau, d.v_th, d.soft_reset = 2.0, 0.1, 1
    if W is not None:
        d.psn_w, d.psn_b = W.data_ptr(), b.data_ptr()
    return d


def psn_wb(T, seed):
    return dev(rnd((T, T), seed, -0.5, 0.5)), dev(rnd((T,), seed + 1, -0.2, 0.2))


@pytest.mark.parametrize("u8", [False, True])
def test_forward_entry_points(u8):
    L, dt = hip.lib(), hip.SDF_U8 if u8 else hip.SDF_F32
    for T in T_STREAM:
        x, _ = xg(T, 10 + T)
        W, b = psn_wb(T, 40 + T)
        name = [("neuron_kernel<%d>(" % T, WGS)]
        check(lambda o: (L.sdf_lif_fwd(x.data_ptr(), o, None, T, N, 2.0, 0.1, 1, 0.0, dt, stream()), []), T * N, name, u8)
        check(lambda o: (L.sdf_psn_fwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), o, T, N, dt, stream()), []), T * N, name, u8)
        check(lambda o: (L.sdf_neuron_fwd(C.byref(neuron_desc(x, o, T, hip.SDF_PSN, u8, W, b)), stream()), []), T * N, name, u8)
        check(lambda o: (L.sdf_neuron_fwd(C.byref(neuron_desc(x, o, T, hip.SDF_IF, u8)), stream()), []), T * N, name, u8)
    x, _ = xg(3, 7)                                                      # a T outside the list: the runtime-T kernel
    check(lambda o: (L.sdf_neuron_fwd(C.byref(neuron_desc(x, o, 3, u8=u8)), stream()), []), 3 * N, [("neuron_kernel<0>(", WGS)], u8)


@pytest.mark.parametrize("u8", [False, True])
def test_neuron_multi_fwd(u8):
    """Two descriptors, the second writing behind the first: one launch of 2 + 2 workgroups for a T of the multi list, else one
    launch each."""
    L, esz = hip.lib(), 1 if u8 else 4
    for T in T_STREAM:
        xa, xb = xg(T, 70 + T)

        def call(o):
            descs = (hip.NeuronDesc * 2)(neuron_desc(xa, o, T, u8=u8), neuron_desc(xb, o + T * N * esz, T, hip.SDF_IF, u8))
            return L.sdf_neuron_multi_fwd(descs, 2, stream()), []
        one = T in T_GLIF
        check(call, 2 * T * N, [("neuron_multi_kernel<%d>(" % T, 2 * WGS)] if one else [("neuron_kernel<%d>(" % T, WGS)] * 2, u8)


def test_lif_family_backward():
    L = hip.lib()
    for T in T_STREAM:
        x, g = xg(T, 100 + T)
        name = [("lif_bwd_kernel<%d, false>(" % T, WGS)]
        for kind in (hip.SDF_LIF, hip.SDF_IF):
            check(lambda o: (L.sdf_lif_bwd(x.data_ptr(), g.data_ptr(), o, T, N, kind, 2.0, 0.1, 1, 0.0, 1, 0, 2.0, stream()), []),
                  T * N, name)
        check(lambda o: (L.sdf_sltt_bwd(x.data_ptr(), g.data_ptr(), o, T, N, 2.0, 0.1, 1, 0.0, 0, 2.0, stream()), []), T * N, name)
        k = dev(torch.tensor([0.4]))
        check(lambda o: (L.sdf_plif_fwd(x.data_ptr(), k.data_ptr(), o, T, N, 0.1, 1, 0.0, stream()), []), T * N,
              [("plif_fwd_kernel<%d>(" % T, WGS)])
        nbytes = L.sdf_plif_bwd_workspace_bytes(T, N)
        assert nbytes == WGS * 4
        ws, gk = f32(WGS), f32(1)
        check(lambda o: (L.sdf_plif_bwd(x.data_ptr(), k.data_ptr(), g.data_ptr(), o, gk.data_ptr(), ws.data_ptr(), nbytes, T, N, 0.1, 1,
                                        0.0, 1, 0, 2.0, stream()), [gk]), T * N,
              [("lif_bwd_kernel<%d, true>(" % T, WGS), ("psn_bwd_finish_kernel(", 1)])


def test_psn_backward():
    """dW / db are reduced in the kernel up to T = 10, 4 neurons per lane up to T = 5 and 2 at T = 8 and 10 (three workgroups over
    514 pairs); without parameter gradients every T runs the 4-wide kernel, with or without dL/dh."""
    L = hip.lib()
    for T in T_STREAM:
        x, g = xg(T, 200 + T)
        W, b = psn_wb(T, 240 + T)
        gh = f32(T * N)
        for h in (None, gh):
            check(lambda o: (L.sdf_psn_bwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), g.data_ptr(), o, None, None, h.data_ptr() if h is not None
                                           else None, None, 0, T, N, 0, 2.0, stream()), [] if h is None else [h]), T * N,
                  [("psn_bwd_kernel<%d, false, 4>(" % T, WGS)])
        if T > 10:
            continue
        vec = 4 if T <= 5 else 2
        wgs = (N // vec + 255) // 256
        nbytes = L.sdf_psn_bwd_workspace_bytes(T, N)
        assert nbytes == wgs * (T * T + T) * 4 and wgs == (2 if vec == 4 else 3)
        ws, gW, gb = f32(nbytes // 4), f32(T * T), f32(T)
        check(lambda o: (L.sdf_psn_bwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), g.data_ptr(), o, gW.data_ptr(), gb.data_ptr(), None,
                                       ws.data_ptr(), nbytes, T, N, 0, 2.0, stream()), [gW, gb]), T * N,
              [("psn_bwd_kernel<%d, true, %d>(" % (T, vec), wgs), ("psn_bwd_finish_kernel(", T * T + T)])


def test_glif():
    L = hip.lib()
    for T in T_GLIF:
        x, g = xg(T, 300 + T)
        tab = dev(rnd((5 + T,), 340 + T, 0.2, 0.8))
        for u8 in (False, True):
            check(lambda o: (L.sdf_glif_fwd(x.data_ptr(), tab.data_ptr(), o, T, N, hip.SDF_U8 if u8 else hip.SDF_F32, stream()), []),
                  T * N, [("glif_fwd_kernel<%d, %s>(" % (T, "true" if u8 else "false"), WGS)], u8)
        nbytes = L.sdf_glif_bwd_workspace_bytes(T, N)
        assert nbytes == WGS * (5 + T) * 4
        ws, gtab = f32(nbytes // 4), f32(5 + T)
        check(lambda o: (L.sdf_glif_bwd(x.data_ptr(), tab.data_ptr(), g.data_ptr(), o, gtab.data_ptr(), ws.data_ptr(), nbytes, T, N, 0,
                                        2.0, stream()), [gtab]), T * N,
              [("glif_bwd_kernel<%d>(" % T, WGS), ("glif_bwd_finish_kernel(", 5 + T)])


def test_qk_gate_train():
    """e and dL/dk go into the guarded buffer; dL/dq (bit-compared between the two calls) beside it."""
    L, n = hip.lib(), ROWS * CC
    for Tq in T_GATE:
        q = dev((rnd((Tq, ROWS, CC), 400 + Tq, 0.0, 1.0) < 0.1).float())
        k = dev((rnd((Tq, ROWS, CC), 410 + Tq, 0.0, 1.0) < 0.3).float())
        ge = dev(rnd((Tq, ROWS, CC), 420 + Tq))
        W, b = psn_wb(Tq, 430 + Tq)
        pk, gq = dev(torch.tensor([0.4])), f32(Tq * n)
        for kind in (hip.SDF_LIF, hip.SDF_IF, hip.SDF_PSN):
            pw, pb = (W.data_ptr(), b.data_ptr()) if kind == hip.SDF_PSN else (None, None)
            check(lambda o: (L.sdf_qk_gate_f32_fwd(q.data_ptr(), k.data_ptr(), o, Tq, ROWS, CC, kind, 2.0, 0.1, 1, 0.0, pw, pb, stream()),
                             []), Tq * n, [("qk_gate_train_kernel<%d, false, false>(" % Tq, GATE_WGS)])
            psn = kind == hip.SDF_PSN
            nbytes = L.sdf_qk_gate_bwd_workspace_bytes(Tq, ROWS, CC) if psn else 0
            assert nbytes == (GATE_WGS * (Tq * Tq + Tq) * 4 if psn else 0)
            ws, gW, gb = (f32(nbytes // 4), f32(Tq * Tq), f32(Tq)) if psn else (None, None, None)
            ptr = lambda t: t.data_ptr() if t is not None else None
            check(lambda o: (L.sdf_qk_gate_bwd(q.data_ptr(), k.data_ptr(), ge.data_ptr(), gq.data_ptr(), o, Tq, ROWS, CC, kind, 2.0, 0.1, 1,
                                               0.0, 1, 0, 2.0, pw, pb, ptr(gW), ptr(gb), ptr(ws), nbytes, stream()),
                             [gq] + ([gW, gb] if psn else [])), Tq * n,
                  [("qk_gate_train_kernel<%d, true, false>(" % Tq, GATE_WGS)] + ([("gate_finish_kernel(", Tq * Tq + Tq)] if psn else []))
        check(lambda o: (L.sdf_qk_gate_plif_f32_fwd(q.data_ptr(), k.data_ptr(), o, pk.data_ptr(), Tq, ROWS, CC, 0.1, 1, 0.0, stream()), []),
              Tq * n, [("qk_gate_train_kernel<%d, false, true>(" % Tq, GATE_WGS)])
        nbytes = L.sdf_qk_gate_plif_bwd_workspace_bytes(Tq, ROWS, CC)
        assert nbytes == GATE_WGS * 4
        ws, gpk = f32(1), f32(1)
        check(lambda o: (L.sdf_qk_gate_plif_bwd(q.data_ptr(), k.data_ptr(), ge.data_ptr(), gq.data_ptr(), o, pk.data_ptr(), gpk.data_ptr(),
                                                ws.data_ptr(), nbytes, Tq, ROWS, CC, 0.1, 1, 0.0, 1, 0, 2.0, stream()), [gq, gpk]),
              Tq * n, [("qk_gate_train_kernel<%d, true, true>(" % Tq, GATE_WGS), ("gate_finish_kernel(", 1)])
