"""ctypes binding of libsdformerflow_hip.so (the C ABI declared in include/sdformerflow_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every compute call goes through the
C ABI with raw pointers.  `SIGNATURES` declares the return and argument types of every entry point, so
call sites pass plain Python ints, floats, pointers (`_ptr`, `None`) and descriptors (`C.byref(desc)`
or an array of them).  There is NO CPU fallback: if the library is missing or a tensor is not on
the GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import inspect
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SDF_HIP_LIB selects a DIAGNOSTIC build (tools/stamp_pp.sh, tools/gemm_ablate.sh build theirs beside the product library,
# never over it); unset = the product library
LIB_PATH = os.environ.get("SDF_HIP_LIB") or os.path.join(_HERE, "csrc", "libsdformerflow_hip.so")

SDF_F32, SDF_U8 = 0, 1
SDF_LIF, SDF_PSN, SDF_IF = 0, 1, 2
KIND = {"lif": SDF_LIF, "psn": SDF_PSN, "if": SDF_IF}


class SdfError(RuntimeError):
    """`rc` = the C ABI's return code when the error came from an entry point (negative: SDF_E_* argument refusal before any launch,
    positive: hipError_t), else None."""

    def __init__(self, msg, rc=None):
        super().__init__(msg)
        self.rc = rc


class ReplicaGeometryError(SdfError):
    """A replica launch sequence cannot serve this geometry (the window count per sample is not a multiple of the window depth at some
    stage): the caller runs the samples one by one - same results."""


# The diagnostic SDF_* switches are read ONCE - at import here, at the first call that asks for one in the
# library (csrc/switches.hip) - not per call.  A harness that changes the environment afterwards says so: reload_switches().
_SW = {k: v for k, v in os.environ.items() if k.startswith("SDF_")}


def sw(name, default=None):
    """Value of the switch SDF_<...> as of import / the last reload_switches() (a drop-in for os.environ.get)."""
    return _SW.get(name, default)


def reload_switches():
    """Re-read every SDF_* switch from the environment, on both sides of the C ABI (tests/conftest.py calls it around setenv)."""
    _SW.clear()
    _SW.update({k: v for k, v in os.environ.items() if k.startswith("SDF_")})
    if _lib is not None:
        _lib.sdf_switches_reload()


class scoped_switches:
    """`with hip.scoped_switches(SDF_CONV_WRES="0"):` - set (value None: unset) diagnostic switches for a block of calls and restore
    them afterwards, refreshing the tables both times (A/B legs of tests and tools)."""

    def __init__(self, **kw):
        self._kw = kw

    def __enter__(self):
        self._old = {k: os.environ.get(k) for k in self._kw}
        for k, v in self._kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        reload_switches()
        return self

    def __exit__(self, *exc):
        for k, v in self._old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        reload_switches()


class NeuronDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("v_last", C.c_void_p),
                ("T", C.c_int32), ("out_dtype", C.c_int32),
                ("nb", C.c_int64), ("ni", C.c_int64),
                ("x_sb", C.c_int64), ("x_st", C.c_int64),
                ("o_sb", C.c_int64), ("o_st", C.c_int64),
                ("rowmap", C.c_void_p), ("rowlen", C.c_int32), ("kind", C.c_int32),
                ("alpha", C.c_void_p), ("beta", C.c_void_p), ("C", C.c_int32), ("inner", C.c_int32),
                ("add", C.c_void_p), ("add_st", C.c_int64), ("add_period", C.c_int64),
                ("tau", C.c_float), ("v_th", C.c_float), ("v_reset", C.c_float), ("soft_reset", C.c_int32),
                ("psn_w", C.c_void_p), ("psn_b", C.c_void_p),
                ("nrep", C.c_int64), ("x_srep", C.c_int64), ("o_srep", C.c_int64)]


class SpikeGemmDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("Wp", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int64), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int64), ("ldo", C.c_int64), ("nsplit", C.c_int32),
                ("bias", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p),
                ("resid", C.c_void_p), ("out_rowmap", C.c_void_p),
                ("zg_nH", C.c_int32), ("zg_T", C.c_int32), ("zg_B", C.c_int32), ("zg_N1", C.c_int32),
                ("sn_T", C.c_int32), ("sn_kind", C.c_int32),
                ("tau", C.c_float), ("v_th", C.c_float), ("v_reset", C.c_float), ("soft_reset", C.c_int32),
                ("psn_w", C.c_void_p), ("psn_b", C.c_void_p),
                ("pos_count", C.c_int64), ("pos_inner", C.c_int64), ("pos_ostride", C.c_int64), ("t_stride", C.c_int64),
                ("add", C.c_void_p), ("add_prows", C.c_int64), ("out_spike", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("acc_scale", C.c_float), ("out_rows", C.c_int64),
                ("col_scale", C.c_void_p), ("zg_rep", C.c_int32)]


class SpikeConvDesc(C.Structure):
    _fields_ = [("g", SpikeGemmDesc), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("OH", C.c_int32),
                ("OW", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32), ("sy", C.c_int32), ("sx", C.c_int32),
                ("dy", C.c_int32 * 3), ("dx", C.c_int32 * 3)]


class HeadConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
                ("sn_kind", C.c_int32), ("tau", C.c_float), ("v_th", C.c_float), ("v_reset", C.c_float),
                ("soft_reset", C.c_int32), ("psn_w", C.c_void_p), ("psn_b", C.c_void_p),
                ("x_sb", C.c_int64), ("x_st", C.c_int64), ("x_sy", C.c_int64), ("x_sx", C.c_int64), ("x_sc", C.c_int64 * 4)]


class WinAttnDesc(C.Structure):
    _fields_ = [("mode", C.c_int32), ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("out", C.c_void_p),
                ("B_", C.c_int32), ("nW", C.c_int32), ("nH", C.c_int32), ("N", C.c_int32), ("hd", C.c_int32),
                ("Tq", C.c_int32), ("N1", C.c_int32),
                ("scale", C.c_void_p), ("bias", C.c_void_p), ("mask", C.c_void_p), ("row_map", C.c_void_p), ("pad_qkv", C.c_void_p)]


class WinAttnBwdDesc(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("row_map", C.c_void_p), ("pad_qkv", C.c_void_p), ("dout", C.c_void_p),
                ("scale", C.c_void_p), ("bias", C.c_void_p), ("mask", C.c_void_p), ("dqkv", C.c_void_p), ("d_pad", C.c_void_p),
                ("d_scale", C.c_void_p), ("d_bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("B_", C.c_int32), ("nW", C.c_int32), ("nH", C.c_int32), ("N", C.c_int32), ("hd", C.c_int32)]


class WinAttnSewBwdDesc(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("dout", C.c_void_p), ("scale", C.c_void_p),
                ("bias", C.c_void_p), ("mask", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
                ("d_bias", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("B_", C.c_int32), ("nW", C.c_int32), ("nH", C.c_int32), ("Tq", C.c_int32), ("N1", C.c_int32), ("hd", C.c_int32)]


class AnnMlpBlockDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int64), ("C", C.c_int32), ("Ch", C.c_int32),
                ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("w1", C.c_void_p), ("b1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p)]


class SpikeDeconvDesc(C.Structure):
    _fields_ = [("spikes", C.c_void_p), ("digits", C.c_void_p), ("cscale", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p),
                ("out", C.c_void_p), ("imgs", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("Cout", C.c_int32)]


class AnnAttnBlockDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("row_map", C.c_void_p),
                ("B_", C.c_int32), ("nW", C.c_int32), ("nH", C.c_int32), ("N", C.c_int32), ("C", C.c_int32), ("rows", C.c_int64),
                ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("ln_eps", C.c_float),
                ("wqkv", C.c_void_p), ("qkv_bias", C.c_void_p), ("scale", C.c_void_p), ("table", C.c_void_p),
                ("wproj", C.c_void_p), ("proj_bias", C.c_void_p)]


class DenseConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p), ("resid", C.c_void_p),
                ("out", C.c_void_p), ("imgs", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("cin_records", C.c_int32),
                ("N", C.c_int32), ("relu", C.c_int32), ("out_f32", C.c_int32), ("x_records", C.c_int32), ("acc_scale", C.c_float)]


class DenseLinearDesc(C.Structure):
    _fields_ = [("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("resid", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("gelu", C.c_int32),
                ("cv_H", C.c_int32), ("cv_W", C.c_int32), ("cv_C", C.c_int32), ("cv_stride", C.c_int32), ("cv_OH", C.c_int32),
                ("cv_OW", C.c_int32), ("out_T", C.c_int32), ("acc_scale", C.c_float)]


class LinearDwDesc(C.Structure):
    _fields_ = [("dy", C.c_void_p), ("x", C.c_void_p), ("dw", C.c_void_p), ("partial", C.c_void_p),
                ("M", C.c_int64), ("N", C.c_int32), ("K", C.c_int32), ("nsplit", C.c_int32), ("cv_C", C.c_int32), ("cv_Wp", C.c_int32)]


class LinearTrainDesc(C.Structure):
    _fields_ = [("a", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("mode", C.c_int32), ("cv_C", C.c_int32), ("cv_Wp", C.c_int32)]


class LaunchRecord(C.Structure):
    _fields_ = [("kernel", C.c_char * 192), ("workgroups", C.c_uint32), ("threads", C.c_uint32), ("lds_bytes", C.c_uint32), ("us", C.c_float)]


class NeuronCfg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("tau", C.c_float), ("v_th", C.c_float), ("v_reset", C.c_float),
                ("soft_reset", C.c_int32), ("psn_w", C.c_void_p), ("psn_b", C.c_void_p)]


class QkAttnDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("slice_map", C.c_void_p), ("B_", C.c_int64), ("x_rows", C.c_int64),
                ("Tq", C.c_int32), ("N1", C.c_int32), ("C", C.c_int32), ("nH", C.c_int32), ("nsplit", C.c_int32),
                ("qk_planes", C.c_void_p), ("qk_alpha", C.c_void_p), ("qk_beta", C.c_void_p), ("qk_add", C.c_void_p),
                ("qk_acc_scale", C.c_float),
                ("q_planes", C.c_void_p), ("q_alpha", C.c_void_p), ("q_beta", C.c_void_p), ("q_acc_scale", C.c_float),
                ("k_planes", C.c_void_p), ("k_alpha", C.c_void_p), ("k_beta", C.c_void_p), ("k_add", C.c_void_p),
                ("k_acc_scale", C.c_float),
                ("p_planes", C.c_void_p), ("p_bias", C.c_void_p), ("p_alpha", C.c_void_p), ("p_beta", C.c_void_p),
                ("p_acc_scale", C.c_float),
                ("sn_proj", NeuronCfg), ("sn_q", NeuronCfg), ("sn_k", NeuronCfg), ("sn2_q", NeuronCfg),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("gemm_workspace", C.c_void_p), ("gemm_workspace_bytes", C.c_int64), ("flags", C.c_int32),
                ("x_src", C.c_void_p), ("xB", C.c_int32), ("xD", C.c_int32), ("xHW", C.c_int64), ("emit_s1", C.c_void_p),
                ("emit_sn", NeuronCfg),
                ("qk_digits", C.c_void_p), ("qk_cscale", C.c_void_p), ("q_digits", C.c_void_p), ("q_cscale", C.c_void_p),
                ("k_digits", C.c_void_p), ("k_cscale", C.c_void_p), ("p_digits", C.c_void_p), ("p_cscale", C.c_void_p),
                ("rep_windows", C.c_int32)]


class MsMlpDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("B", C.c_int32), ("D", C.c_int32), ("HW", C.c_int64), ("C", C.c_int32), ("Ch", C.c_int32),
                ("nsplit", C.c_int32),
                ("fc1_planes", C.c_void_p), ("fc1_alpha", C.c_void_p), ("fc1_beta", C.c_void_p), ("fc1_acc_scale", C.c_float),
                ("fc2_planes", C.c_void_p), ("fc2_alpha", C.c_void_p), ("fc2_beta", C.c_void_p), ("fc2_acc_scale", C.c_float),
                ("sn1", NeuronCfg), ("sn2", NeuronCfg),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("gemm_workspace", C.c_void_p), ("gemm_workspace_bytes", C.c_int64), ("flags", C.c_int32), ("s1_in", C.c_void_p),
                ("fc1_digits", C.c_void_p), ("fc1_cscale", C.c_void_p), ("fc2_digits", C.c_void_p), ("fc2_cscale", C.c_void_p),
                ("emit_next", C.c_void_p), ("emit_sn", NeuronCfg), ("fc2_tiled", C.c_void_p)]


class MsMergeDesc(C.Structure):
    _fields_ = [("spikes", C.c_void_p), ("digits", C.c_void_p), ("cscale", C.c_void_p), ("alpha", C.c_void_p), ("beta", C.c_void_p),
                ("out", C.c_void_p), ("B", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("N", C.c_int32)]


class PointwiseConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("imgs", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("Cin", C.c_int32), ("N", C.c_int32), ("stride", C.c_int32), ("OH", C.c_int32), ("OW", C.c_int32)]


class PredHeadDesc(C.Structure):
    _fields_ = [("z", C.c_void_p), ("B", C.c_int32), ("D", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("Cin", C.c_int32),
                ("sn_pred", NeuronCfg), ("wgt", C.c_void_p), ("bias", C.c_void_p), ("pred", C.c_void_p), ("flow", C.c_void_p),
                ("H", C.c_int32), ("W", C.c_int32), ("next_spikes", C.c_void_p), ("next_ld", C.c_int32), ("next_z_off", C.c_int32),
                ("next_pred_off", C.c_int32), ("next_zero_off", C.c_int32), ("next_zero_len", C.c_int32), ("sn_next", NeuronCfg),
                ("keep_spikes", C.c_void_p)]


class EventVoxelDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("p", C.c_void_p), ("rectify_map", C.c_void_p),
                ("offsets", C.c_void_p), ("t_range", C.c_void_p), ("keys", C.c_void_p), ("keys_sorted", C.c_void_p), ("order", C.c_void_p),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_events", C.c_int64),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32),
                ("map_h", C.c_int32), ("map_w", C.c_int32), ("xy_dtype", C.c_int32), ("mode", C.c_int32), ("norm", C.c_int32),
                ("use_spike_th", C.c_int32), ("spike_th", C.c_float)]


class EventVoxelTbDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("t_scale", C.c_void_p), ("p", C.c_void_p),
                ("offsets", C.c_void_p), ("keys", C.c_void_p), ("keys_sorted", C.c_void_p), ("order", C.c_void_p), ("out", C.c_void_p),
                ("event_mask", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_events", C.c_int64),
                ("n_lists", C.c_int32), ("lists_per_sample", C.c_int32), ("nb", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("crop_h", C.c_int32), ("crop_w", C.c_int32), ("crop_oy", C.c_int32), ("crop_ox", C.c_int32), ("xy_dtype", C.c_int32),
                ("normalize", C.c_int32), ("mode", C.c_int32), ("norm", C.c_int32), ("use_spike_th", C.c_int32), ("spike_th", C.c_float)]


class EventIweDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("p", C.c_void_p), ("flow", C.c_void_p), ("rectify_map", C.c_void_p),
                ("offsets", C.c_void_p), ("t_range", C.c_void_p), ("keys", C.c_void_p), ("keys_sorted", C.c_void_p), ("order", C.c_void_p),
                ("out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_events", C.c_int64),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32), ("crop_oy", C.c_int32),
                ("crop_ox", C.c_int32), ("map_h", C.c_int32), ("map_w", C.c_int32), ("xy_dtype", C.c_int32), ("mode", C.c_int32),
                ("scale", C.c_float), ("t_ref", C.c_float), ("win_a", C.c_float), ("win_b", C.c_float)]


class IweStatsDesc(C.Structure):
    _fields_ = [("iwe", C.c_void_p), ("table", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32)]


class FlowMetricsDesc(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("label", C.c_void_p), ("valid", C.c_void_p), ("event_mask", C.c_void_p), ("table", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("row0", C.c_int32), ("rows", C.c_int32), ("flow_scaling", C.c_float)]


FLOW_LOSS_MAX_LEVELS = 8                 # SDF_FLOW_LOSS_MAX_LEVELS


class FlowLossDesc(C.Structure):
    _fields_ = [("pred", C.c_void_p * 8), ("grad", C.c_void_p * 8), ("h", C.c_int32 * 8), ("w", C.c_int32 * 8), ("T", C.c_int32 * 8),
                ("label", C.c_void_p), ("mask", C.c_void_p), ("n_valid", C.c_void_p), ("loss", C.c_void_p), ("records", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("levels", C.c_int32), ("B", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("dtype", C.c_int32), ("flow_scaling", C.c_float), ("lambda_mod", C.c_float)]


class PrepareChunkDesc(C.Structure):
    _fields_ = [("voxel", C.c_void_p), ("out", C.c_void_p), ("event_mask", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("B", C.c_int32), ("bins", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32),
                ("crop_h", C.c_int32), ("crop_w", C.c_int32), ("crop_oy", C.c_int32), ("crop_ox", C.c_int32), ("norm", C.c_int32),
                ("per_sample", C.c_int32), ("use_spike_th", C.c_int32), ("spike_th", C.c_float)]


AUGMENT_MAX_B = 64                       # SDF_AUGMENT_MAX_B


class AugmentResizeDesc(C.Structure):
    _fields_ = [("vox_old", C.c_void_p), ("vox_new", C.c_void_p), ("flow", C.c_void_p), ("scale_x", C.c_void_p), ("scale_y", C.c_void_p),
                ("out", C.c_void_p), ("label_out", C.c_void_p), ("mask_out", C.c_void_p), ("event_mask", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("B", C.c_int32), ("bins", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32),
                ("num_chunks", C.c_int32), ("norm", C.c_int32), ("per_sample", C.c_int32), ("use_spike_th", C.c_int32),
                ("mask_events", C.c_int32), ("spike_th", C.c_float),
                ("resized", C.c_int32 * 64), ("rh", C.c_int32 * 64), ("rw", C.c_int32 * 64), ("oy", C.c_int32 * 64), ("ox", C.c_int32 * 64),
                ("flags", C.c_int32 * 64)]


class AugmentChunkDesc(C.Structure):
    _fields_ = [("voxel", C.c_void_p), ("label", C.c_void_p), ("valid", C.c_void_p), ("drop_u", C.c_void_p), ("out", C.c_void_p),
                ("label_out", C.c_void_p), ("mask_out", C.c_void_p), ("event_mask", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("seed", C.c_int64), ("offset", C.c_int64),
                ("B", C.c_int32), ("bins", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32),
                ("valid_is_u8", C.c_int32), ("norm", C.c_int32), ("per_sample", C.c_int32), ("use_spike_th", C.c_int32),
                ("mask_events", C.c_int32), ("spike_th", C.c_float),
                ("oy", C.c_int32 * 64), ("ox", C.c_int32 * 64), ("flags", C.c_int32 * 64), ("drop_q", C.c_float * 64)]


class FlowImageDesc(C.Structure):
    _fields_ = [("flow", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class FlowSubmissionDesc(C.Structure):
    _fields_ = [("flow", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class EventImageDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("chunk_vis", C.c_void_p), ("bounds", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int32), ("bins", C.c_int32), ("Hs", C.c_int32), ("Ws", C.c_int32), ("crop_h", C.c_int32), ("crop_w", C.c_int32),
                ("crop_oy", C.c_int32), ("crop_ox", C.c_int32), ("mode", C.c_int32), ("stage", C.c_int32)]


class SpikeCountDesc(C.Structure):
    _fields_ = [("spikes", C.c_void_p), ("outer", C.c_int64), ("T", C.c_int), ("rows", C.c_int64), ("C", C.c_int),
                ("row_stride", C.c_int64), ("counts", C.c_void_p)]


class SpikeCountSegDesc(C.Structure):
    _fields_ = [("spikes", C.c_void_p), ("s_out", C.c_int64), ("T", C.c_int), ("s_in", C.c_int64), ("rows", C.c_int64), ("C", C.c_int),
                ("row_stride", C.c_int64), ("counts", C.c_void_p), ("sample_pitch", C.c_int64)]


class MembraneStatsDesc(C.Structure):
    _fields_ = [("v", C.c_void_p), ("outer", C.c_int64), ("T", C.c_int), ("rows", C.c_int64), ("C", C.c_int),
                ("row_stride", C.c_int64), ("table", C.c_void_p), ("bins", C.c_int), ("lo", C.c_float), ("hi", C.c_float),
                ("inv_width", C.c_float)]


class GradStatsDesc(C.Structure):
    _fields_ = [("flat", C.c_void_p), ("n", C.c_int64), ("seg_host", C.c_void_p), ("seg", C.c_void_p), ("nseg", C.c_int32),
                ("row0", C.c_int32), ("rows", C.c_int32), ("table", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class AdamwRow(C.Structure):
    _fields_ = [("param", C.c_void_p), ("offset", C.c_int64), ("length", C.c_int64), ("decay", C.c_float), ("w1", C.c_float),
                ("beta2", C.c_float), ("w2", C.c_float), ("neg_step_size", C.c_float), ("bc2_sqrt", C.c_float), ("eps", C.c_float),
                ("active", C.c_int32)]


class AdamwDesc(C.Structure):
    _fields_ = [("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64), ("rows_host", C.c_void_p),
                ("rows", C.c_void_p), ("nseg", C.c_int32), ("coef", C.c_void_p)]


class LossScaleState(C.Structure):
    _fields_ = [("scale", C.c_float), ("growth_tracker", C.c_int32), ("inv_scale", C.c_float), ("found_inf", C.c_int32),
                ("skipped", C.c_int64)]


class GradScaleDesc(C.Structure):
    _fields_ = [("flat", C.c_void_p), ("n", C.c_int64), ("seg_host", C.c_void_p), ("seg", C.c_void_p), ("nseg", C.c_int32),
                ("mask", C.c_void_p), ("coef", C.c_void_p)]


class GradClipScaleDesc(C.Structure):
    _fields_ = [("table", C.c_void_p), ("rows", C.c_int32), ("mask", C.c_void_p), ("max_norm", C.c_float), ("coef", C.c_void_p),
                ("record", C.c_void_p), ("state", C.c_void_p), ("growth_factor", C.c_float), ("backoff_factor", C.c_float),
                ("growth_interval", C.c_int32), ("clip_unscaled", C.c_int32), ("update", C.c_int32)]


# The C ABI in header order, a family of entry points per line: name -> (restype, argtypes).  lib() declares every one, so ctypes converts
# plain Python ints / floats / pointers itself and refuses a wrong argument count or type at the call (an int too wide for its C type is
# still truncated).  tests/test_abi_cpu.py checks the table and the Structure mirrors against include/sdformerflow_hip.h.
_i, _i64, _f, _p, _P = C.c_int, C.c_int64, C.c_float, C.c_void_p, C.POINTER
SIGNATURES = {
    "sdf_version": (_i, ()), "sdf_switches_reload": (None, ()),
    "sdf_launch_log": (None, (_i,)), "sdf_launch_log_read": (_i, (_P(LaunchRecord), _i)),
    "sdf_lif_fwd": (_i, (_p, _p, _p, _i, _i64, _f, _f, _i, _f, _i, _p)),
    "sdf_psn_fwd": (_i, (_p, _p, _p, _p, _i, _i64, _i, _p)),
    "sdf_lif_bwd": (_i, (_p, _p, _p, _i, _i64, _i, _f, _f, _i, _f, _i, _i, _f, _p)),
    "sdf_psn_bwd_workspace_bytes": (_i64, (_i, _i64)),
    "sdf_psn_bwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i64, _i, _f, _p)),
    "sdf_plif_fwd": (_i, (_p, _p, _p, _i, _i64, _f, _i, _f, _p)), "sdf_plif_bwd_workspace_bytes": (_i64, (_i, _i64)),
    "sdf_plif_bwd": (_i, (_p, _p, _p, _p, _p, _p, _i64, _i, _i64, _f, _i, _f, _i, _i, _f, _p)),
    "sdf_sltt_bwd": (_i, (_p, _p, _p, _i, _i64, _f, _f, _i, _f, _i, _f, _p)),
    "sdf_glif_fwd": (_i, (_p, _p, _p, _i, _i64, _i, _p)), "sdf_glif_bwd_workspace_bytes": (_i64, (_i, _i64)),
    "sdf_glif_bwd": (_i, (_p, _p, _p, _p, _p, _p, _i64, _i, _i64, _i, _f, _p)),
    "sdf_bn_train_workspace_bytes": (_i64, (_i64, _i)),
    "sdf_bn_train_fwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _f, _f, _p, _i64, _p)),
    "sdf_bn_train_bwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _p, _i64, _p)),
    "sdf_bn_train_nchw_fwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _f, _f, _p, _i64, _p)),
    "sdf_bn_train_nchw_bwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _p, _i64, _p)),
    "sdf_qk_gate_f32_fwd": (_i, (_p, _p, _p, _i, _i64, _i, _i, _f, _f, _i, _f, _p, _p, _p)),
    "sdf_qk_gate_bwd_workspace_bytes": (_i64, (_i, _i64, _i)),
    "sdf_qk_gate_bwd": (_i, (_p, _p, _p, _p, _p, _i, _i64, _i, _i, _f, _f, _i, _f, _i, _i, _f, _p, _p, _p, _p, _p, _i64, _p)),
    "sdf_qk_gate_plif_f32_fwd": (_i, (_p, _p, _p, _p, _i, _i64, _i, _f, _i, _f, _p)),
    "sdf_qk_gate_plif_bwd_workspace_bytes": (_i64, (_i, _i64, _i)),
    "sdf_qk_gate_plif_bwd": (_i, (_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i64, _i, _f, _i, _f, _i, _i, _f, _p)),
    "sdf_neuron_fwd": (_i, (_P(NeuronDesc), _p)), "sdf_neuron_multi_fwd": (_i, (_P(NeuronDesc), _i, _p)),
    "sdf_glif_neuron_fwd": (_i, (_P(NeuronDesc), _p, _p)), "sdf_neuron_vseq_fwd": (_i, (_P(NeuronDesc), _p, _p)),
    "sdf_split_weight_i8x3": (_i, (_p, _p, _p, _i, _i, _p)), "sdf_tile_weight_i8x3": (_i, (_p, _p, _i, _i, _p)),
    "sdf_spike_gemm_fwd": (_i, (_P(SpikeGemmDesc), _p)),
    "sdf_spike_gemm_bn_fwd": (_i, (_p, _p, _i, _f, _p, _p, _p, _i64, _i, _i, _p)),
    "sdf_window_slice_map": (_i, (_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p)),
    "sdf_rows_gather_fwd": (_i, (_p, _p, _p, _i64, _i, _p)), "sdf_rows_scatter_fwd": (_i, (_p, _p, _p, _i64, _i, _p)),
    "sdf_window_zsrc_map": (_i, (_p, _i64, _i, _i, _i, _p, _p)), "sdf_qk_attn_workspace_bytes": (_i64, (_i64, _i, _i, _i)),
    "sdf_qk_attn_fwd": (_i, (_P(QkAttnDesc), _p)), "sdf_qk_attn_is_wide": (_i, (_P(QkAttnDesc),)),
    "sdf_ms_mlp_workspace_bytes": (_i64, (_i64, _i, _i)), "sdf_ms_mlp_fwd": (_i, (_P(MsMlpDesc), _p)),
    "sdf_ms_mlp_is_wide": (_i, (_P(MsMlpDesc),)),
    "sdf_ms_patch_merge_fwd": (_i, (_P(MsMergeDesc), _p)), "sdf_spike_deconv3x3s2_fwd": (_i, (_P(SpikeDeconvDesc), _p)),
    "sdf_spike_conv2d_fwd": (_i, (_P(SpikeConvDesc), _p)), "sdf_spike_conv2d_multi_fwd": (_i, (_P(SpikeConvDesc), _i, _p)),
    "sdf_split_weight_bf16": (_i, (_p, _p, _i64, _i, _p)), "sdf_split_weight_f16x2": (_i, (_p, _p, _i64, _f, _p)),
    "sdf_qk_gate_fwd": (_i, (_p, _p, _p, _i, _i64, _i, _i, _f, _f, _f, _i, _p, _p, _p)),
    "sdf_qk_gate_strided_fwd": (_i, (_p, _p, _p, _i, _i64, _i, _i64, _i64, _i, _f, _f, _f, _i, _p, _p, _p)),
    "sdf_qk_gate_glif_fwd": (_i, (_p, _p, _p, _p, _p, _i, _i64, _i, _i64, _i64, _p)),
    "sdf_head_conv_sn_fwd": (_i, (_P(HeadConvDesc), _p)), "sdf_pointwise_conv_f32_fwd": (_i, (_P(PointwiseConvDesc), _p)),
    "sdf_deconv_col2im_fwd": (_i, (_p, _p, _p, _p, _i, _i, _i, _i, _p)),
    "sdf_flow_out_fwd": (_i, (_p, _p, _i, _i, _i, _i, _i64, _i, _i, _i, _f, _f, _p)),
    "sdf_pred_head_fwd": (_i, (_P(PredHeadDesc), _p)), "sdf_affine_resid_fwd": (_i, (_p, _p, _p, _p, _p, _i64, _i, _i64, _p)),
    "sdf_win_attn_fwd": (_i, (_P(WinAttnDesc), _p)), "sdf_win_attn_large_fwd": (_i, (_P(WinAttnDesc), _p)),
    "sdf_win_attn_scores_fwd": (_i, (_P(WinAttnDesc), _p, _p)),
    "sdf_win_attn_ann_bwd_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_win_attn_ann_bwd": (_i, (_P(WinAttnBwdDesc), _p)),
    "sdf_win_attn_sew_bwd_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_win_attn_sew_bwd": (_i, (_P(WinAttnSewBwdDesc), _p)),
    "sdf_win_attn_large_ann_bwd_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_win_attn_large_ann_bwd": (_i, (_P(WinAttnBwdDesc), _p)),
    "sdf_win_attn_large_sew_bwd_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_win_attn_large_sew_bwd": (_i, (_P(WinAttnSewBwdDesc), _p)),
    "sdf_ann_attn_block_supported": (_i, (_i, _i, _i)), "sdf_ann_attn_block_fwd": (_i, (_P(AnnAttnBlockDesc), _p)),
    "sdf_ann_mlp_block_supported": (_i, (_i, _i)), "sdf_ann_mlp_block_fwd": (_i, (_P(AnnMlpBlockDesc), _p)),
    "sdf_dense_conv3x3_fwd": (_i, (_P(DenseConvDesc), _p)),
    "sdf_pack_planes": (_i, (_p, _p, _i, _i, _i, _i, _p)), "sdf_unpack_planes": (_i, (_p, _p, _i, _i, _i, _i, _p)),
    "sdf_pack_planes_up2": (_i, (_p, _p, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _i, _i, _p)),
    "sdf_pack_planes_zero_up2": (_i, (_p, _p, _i, _i, _i, _i, _i64, _i64, _i64, _i64, _i, _i, _p)),
    "sdf_dense_linear_fwd": (_i, (_P(DenseLinearDesc), _p)),
    "sdf_linear_dw_splits": (_i, (_i64, _i, _i, _i)), "sdf_linear_dw_fwd": (_i, (_P(LinearDwDesc), _p)),
    "sdf_ringed_rows_fwd": (_i, (_p, _p, _i, _i, _i, _i, _p)), "sdf_unring_rows_fwd": (_i, (_p, _p, _p, _i, _i, _i, _i, _p)),
    "sdf_linear_train_fwd": (_i, (_P(LinearTrainDesc), _p)), "sdf_layer_norm_fwd": (_i, (_p, _p, _p, _p, _i64, _i, _f, _p)),
    "sdf_event_voxel_workspace_bytes": (_i64, (_i64, _i, _i, _i, _i, _i, _i)),
    "sdf_event_voxel_keys_fwd": (_i, (_P(EventVoxelDesc), _p)), "sdf_event_voxel_gather_fwd": (_i, (_P(EventVoxelDesc), _p)),
    "sdf_event_voxel_tb_workspace_bytes": (_i64, (_i64, _i, _i, _i, _i, _i, _i, _i, _i, _i)),
    "sdf_event_voxel_tb_keys_fwd": (_i, (_P(EventVoxelTbDesc), _p)), "sdf_event_voxel_tb_gather_fwd": (_i, (_P(EventVoxelTbDesc), _p)),
    "sdf_event_iwe_workspace_bytes": (_i64, (_i64, _i, _i, _i, _i, _i, _i, _i, _i)),
    "sdf_event_iwe_keys_fwd": (_i, (_P(EventIweDesc), _p)), "sdf_event_iwe_gather_fwd": (_i, (_P(EventIweDesc), _p)),
    "sdf_iwe_stats_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_iwe_stats_fwd": (_i, (_P(IweStatsDesc), _p)),
    "sdf_flow_metrics_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_flow_metrics_fwd": (_i, (_P(FlowMetricsDesc), _p)),
    "sdf_flow_loss_workspace_bytes": (_i64, (_i, _i, _i, _i)), "sdf_flow_loss_fwd": (_i, (_P(FlowLossDesc), _p)),
    "sdf_augment_resize_workspace_bytes": (_i64, (_i,)), "sdf_augment_resize_fwd": (_i, (_P(AugmentResizeDesc), _p)),
    "sdf_augment_chunk_workspace_bytes": (_i64, (_i,)), "sdf_augment_chunk_fwd": (_i, (_P(AugmentChunkDesc), _p)),
    "sdf_prepare_chunk_workspace_bytes": (_i64, (_i,)), "sdf_prepare_chunk_fwd": (_i, (_P(PrepareChunkDesc), _p)),
    "sdf_flow_image_workspace_bytes": (_i64, (_i, _i, _i)), "sdf_flow_image_fwd": (_i, (_P(FlowImageDesc), _p)),
    "sdf_flow_submission_fwd": (_i, (_P(FlowSubmissionDesc), _p)), "sdf_event_image_fwd": (_i, (_P(EventImageDesc), _p)),
    "sdf_membrane_stats_fwd": (_i, (_P(MembraneStatsDesc), _p)),
    "sdf_grad_stats_workspace_bytes": (_i64, (_i,)), "sdf_grad_stats_fwd": (_i, (_P(GradStatsDesc), _p)),
    "sdf_grad_clip_coef": (_i, (_p, _i, _p, _f, _p, _p, _p)), "sdf_adamw_step": (_i, (_P(AdamwDesc), _p)),
    "sdf_grad_scale_inplace": (_i, (_P(GradScaleDesc), _p)), "sdf_grad_clip_scale_coef": (_i, (_P(GradClipScaleDesc), _p)),
    "sdf_adamw_step_scaled": (_i, (_P(AdamwDesc), _P(LossScaleState), _p)),
    "sdf_spike_count_seg_fwd": (_i, (_P(SpikeCountSegDesc), _p)),
    "sdf_spike_count_fwd": (_i, (_P(SpikeCountDesc), _p)),
}


_lib = None
_PROF = None            # bench.py's per-call profile: a list of (entry point, note, start event, end event) while profile_calls() is active
_NOTE = {}


class _TimedLib:
    """The library with every `*_fwd` entry point bracketed by two HIP events on the stream it launches on (profile_calls())."""

    def __init__(self, cdll):
        self._c = cdll

    def __getattr__(self, name):
        f = getattr(self._c, name)
        if not name.endswith("_fwd"):
            return f

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            note = dict(_NOTE)
            _NOTE.clear()
            e0.record()
            rc = f(*a)
            e1.record()
            _PROF.append((name, note, e0, e1))
            return rc
        return timed


def _note(**kw):
    """What the next C-ABI call computes (algorithmic flop / bytes, shape) - kept only while a profile is being taken."""
    if _PROF is not None:
        _NOTE.update(kw)


class profile_calls:
    """`with hip.profile_calls() as rec:` - every C-ABI `*_fwd` call inside is timed with HIP events on its own stream; afterwards
    `rec.rows()` = [(entry point, note dict, microseconds)] in call order (bench.py: `roofline.by_time`)."""

    def __enter__(self):
        global _PROF
        lib()
        _PROF = []
        return self

    def __exit__(self, *exc):
        global _PROF
        torch.cuda.synchronize()
        self._rows = [(n, note, e0.elapsed_time(e1) * 1e3) for n, note, e0, e1 in _PROF]
        _PROF = None
        _NOTE.clear()

    def rows(self):
        return self._rows


class launch_log:
    """`with hip.launch_log() as log:` - every kernel launch the library makes inside is timed with HIP events on its own stream
    (sdf_launch_log); afterwards `log.rows` = [(kernel name, workgroups, threads per workgroup, dynamic LDS bytes, microseconds)] in
    launch order.  workgroups x microseconds / 256 = the launch's chip time.  Eager launches only (not under graph capture)."""

    def __enter__(self):
        lib().sdf_launch_log(1)
        return self

    def __exit__(self, *exc):
        c = _lib
        c.sdf_launch_log(0)
        n = c.sdf_launch_log_read(None, 0)
        buf = (LaunchRecord * max(n, 1))()
        c.sdf_launch_log_read(buf, n)
        self.rows = [(buf[i].kernel.decode(errors="replace"), int(buf[i].workgroups), int(buf[i].threads), int(buf[i].lds_bytes), float(buf[i].us))
                     for i in range(n)]


def lib():
    """Load the shared library once; fail loudly when it is absent."""
    global _lib
    if _lib is not None and _PROF is not None:
        return _TimedLib(_lib)
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SdfError(f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(sdformerflow_amd/csrc/build.sh); there is no CPU fallback")
        cdll = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            f = getattr(cdll, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = cdll
    return _lib


E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4          # include/sdformerflow_hip.h: SDF_E_*


def _check(rc, what):
    if rc != 0:
        kind = "argument error" if rc < 0 else "hipError_t"
        raise SdfError(f"{what} failed: {kind} {rc}", rc=rc)


def _ptr(t, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise SdfError("HIP path needs device tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise SdfError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _reset(v_reset):
    """(soft_reset, v_reset) as the C ABI takes them for a neuron's v_reset (None: soft reset)."""
    return (1, 0.0) if v_reset is None else (0, float(v_reset))


_WS = {}


def workspace(device, nbytes=96 << 20):
    """One caller-owned scratch buffer per (device, stream) for the split-K path of the spike matmul / conv kernels:
    forwards running concurrently on different streams must not share partial sums."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    if key not in _WS or _WS[key].numel() < nbytes:
        _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return _WS[key]


def _set_ws(g, like):
    ws = workspace(like.device)
    g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel()


class NeuronParams:
    """Neuron hyper-parameters (the YAML `spiking_neuron` block) plus PSN weights when kind == 'psn'."""

    def __init__(self, kind="lif", tau=2.0, v_th=1.0, v_reset=None, psn_w=None, psn_b=None):
        self.kind, self.tau, self.v_th, self.v_reset = kind, float(tau), float(v_th), v_reset
        self.psn_w, self.psn_b = psn_w, psn_b


class GlifParams(NeuronParams):
    """A GLIF node (the reference's GatedLIFNode) as the kernels take it: `tab` = [L, Dk, g, R, th, c_0 .. c_{T-1}], 5 + T fp32 on the
    device.  No fused epilogue has a GLIF form: `neuron_fwd` sends it to the general GLIF launch, every fused entry point refuses it."""

    def __init__(self, tab):
        super().__init__("glif")
        self.tab = tab


def _neuron_desc(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, p: NeuronParams, rowmap=None, rowlen=0,
                 alpha=None, beta=None, Cch=0, inner=1, add=None, add_st=0, add_period=0, v_last=None, rep=None):
    d = NeuronDesc()
    if rep is not None:
        d.nrep, d.x_srep, d.o_srep = rep                          # (count, stride in x, stride in out) of the outermost dimension
    d.x, d.out, d.v_last = _ptr(x, torch.float32), _ptr(out), _ptr(v_last, torch.float32)
    d.T = T
    d.out_dtype = SDF_F32 if out.dtype == torch.float32 else SDF_U8
    if out.dtype not in (torch.float32, torch.uint8):
        raise SdfError(f"spike dtype {out.dtype} unsupported")
    d.nb, d.ni, d.x_sb, d.x_st, d.o_sb, d.o_st = nb, ni, x_sb, x_st, o_sb, o_st
    d.rowmap, d.rowlen = _ptr(rowmap, torch.int32), rowlen
    d.kind = KIND[p.kind]
    d.alpha, d.beta, d.C, d.inner = _ptr(alpha, torch.float32), _ptr(beta, torch.float32), Cch, inner
    d.add, d.add_st, d.add_period = _ptr(add, torch.float32), add_st, add_period
    d.tau, d.v_th = p.tau, p.v_th
    d.soft_reset, d.v_reset = _reset(p.v_reset)
    d.psn_w, d.psn_b = _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32)
    return d


def neuron_fwd(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, p: NeuronParams, rowmap=None, rowlen=0,
               alpha=None, beta=None, Cch=0, inner=1, add=None, add_st=0, add_period=0, v_last=None, rep=None, v_seq=None):
    """sdf_neuron_fwd: see include/sdformerflow_hip.h for the addressing contract.  `rep` = (count, stride in x, stride in out) of the
    descriptor's outermost dimension.  `v_seq` (fp32, addressed as `out` is, in elements): the call goes to sdf_neuron_vseq_fwd, which
    also writes the membrane after the reset of every step there (LIF / IF; a PSN or GLIF node has no such record)."""
    if p.kind == "glif":
        if v_seq is not None:
            raise SdfError("neuron_fwd: a GLIF node has no v_seq (the reference's GatedLIFNode keeps none either)", rc=E_DTYPE)
        return glif_neuron_fwd(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, p.tab, rowmap, rowlen, alpha, beta, Cch, inner, add, add_st,
                               add_period, v_last, rep)
    d = _neuron_desc(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, p, rowmap, rowlen, alpha, beta, Cch, inner, add, add_st, add_period, v_last,
                     rep)
    if v_seq is not None:
        _note(bytes=T * nb * ni * (8 + out.element_size()), shape=(T, nb * ni))
        _check(lib().sdf_neuron_vseq_fwd(C.byref(d), _ptr(v_seq, torch.float32), _stream()), "sdf_neuron_vseq_fwd")
        return out
    _note(bytes=T * nb * ni * (4 + out.element_size()), shape=(T, nb * ni))
    _check(lib().sdf_neuron_fwd(C.byref(d), _stream()), "sdf_neuron_fwd")
    return out


def glif_neuron_fwd(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, tab, rowmap=None, rowlen=0, alpha=None, beta=None, Cch=0, inner=1,
                    add=None, add_st=0, add_period=0, v_last=None, rep=None):
    """sdf_glif_neuron_fwd: neuron_fwd's addressing with the GLIF recurrence from v = 0, s = 0; `tab` = the node's 5 + T gate table on
    the device; `rep` = (count, stride in x, stride in out) of the descriptor's outermost dimension."""
    if tab.numel() != 5 + T:
        raise SdfError(f"glif_neuron_fwd: the gate table has {tab.numel()} entries, T = {T} needs {5 + T}")
    d = _neuron_desc(x, out, T, nb, ni, x_sb, x_st, o_sb, o_st, NeuronParams(), rowmap, rowlen, alpha, beta, Cch, inner, add, add_st,
                     add_period, v_last, rep)
    _note(bytes=T * nb * ni * (4 + out.element_size()), shape=(T, nb * ni))
    _check(lib().sdf_glif_neuron_fwd(C.byref(d), _ptr(tab, torch.float32), _stream()), "sdf_glif_neuron_fwd")
    return out


def neuron_multi_fwd(calls):
    """sdf_neuron_multi_fwd: `calls` = (args, kwargs) pairs of neuron_fwd - kwargs also takes `rep` = (count, stride in x, stride in out)
    of a descriptor's outermost dimension; one launch when they share T and are at most six."""
    descs = (NeuronDesc * len(calls))(*[_neuron_desc(*a, **k) for a, k in calls])
    _check(lib().sdf_neuron_multi_fwd(descs, len(calls), _stream()), "sdf_neuron_multi_fwd")


def _pad4(*padded):
    """The streaming neuron kernels move 4 neurons per lane: a per-step size that is not a multiple of 4 (e.g. the
    (T', B_, 81, 3) token gate of the QK attention) is run on a zero-padded (T, N4) copy and sliced back.  Decorator: the arguments
    named in `padded` (the first one gives T and N) reach the wrapper contiguous and, where needed, padded; its result - of a tuple
    the first entry, dL/dx - is sliced back to the caller's shape.  Padded columns carry x = 0 and dL/ds = 0, hence dL/dh = 0 at
    every step: they add nothing to the parameter gradients (dL/dk, dL/dtab, dW / db), which pass through as they are."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def wrapper(*args, **kw):
            call = sig.bind(*args, **kw)
            first = call.arguments[padded[0]]
            shape, T, N = first.shape, first.shape[0], first[0].numel()
            for name in padded:
                t = call.arguments[name]
                call.arguments[name] = torch.nn.functional.pad(t.reshape(T, N), (0, -N % 4)) if N % 4 else t.contiguous()
            res = fn(*call.args, **call.kwargs)
            if N % 4 == 0:
                return res
            return (res[0][:, :N].reshape(shape), *res[1:]) if isinstance(res, tuple) else res[:, :N].reshape(shape)
        return wrapper
    return deco


def _ws_f32(nbytes, device):
    """fp32 workspace of at least `nbytes` (what a *_workspace_bytes function asked for) and never empty."""
    return torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=device)


def lif_fwd(x, tau=2.0, v_th=1.0, v_reset=None, out_dtype=torch.float32, return_v=False):
    """Multi-step LIF over dim 0 of a contiguous tensor (sdf_lif_fwd; any per-step size - the library handles N % 4 != 0)."""
    x = x.contiguous()
    T, N = x.shape[0], x[0].numel()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    v = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device) if return_v else None
    rc = lib().sdf_lif_fwd(_ptr(x, torch.float32), _ptr(out), _ptr(v), T, N, tau, v_th, *_reset(v_reset),
                           SDF_F32 if out_dtype == torch.float32 else SDF_U8, _stream())
    _check(rc, "sdf_lif_fwd")
    return (out, v) if return_v else out


@_pad4("x", "grad_spike")
def lif_bwd(x, grad_spike, tau=2.0, v_th=1.0, v_reset=None, detach_reset=True, alpha=2.0, kind="lif"):
    """BPTT through the multi-step LIF / IF over dim 0 (sdf_lif_bwd): dL/dx from x and dL/dspike; ATan surrogate."""
    T, N = x.shape[0], x[0].numel()
    gx = torch.empty_like(x)
    rc = lib().sdf_lif_bwd(_ptr(x, torch.float32), _ptr(grad_spike, torch.float32), _ptr(gx), T, N, KIND[kind], tau, v_th,
                           *_reset(v_reset), 1 if detach_reset else 0, 0, alpha, _stream())
    _check(rc, "sdf_lif_bwd")
    return gx


@_pad4("x")
def plif_fwd(x, k, v_th=1.0, v_reset=None):
    """Multi-step ParametricLIFNode over dim 0 for the training path (sdf_plif_fwd): fp32 spikes; `k` = sigmoid(w), a one-element
    fp32 DEVICE tensor (read by the kernel, never by the host)."""
    T, N = x.shape[0], x[0].numel()
    out = torch.empty_like(x)
    rc = lib().sdf_plif_fwd(_ptr(x, torch.float32), _ptr(k, torch.float32), _ptr(out), T, N, v_th, *_reset(v_reset), _stream())
    _check(rc, "sdf_plif_fwd")
    return out


@_pad4("x", "grad_spike")
def plif_bwd(x, k, grad_spike, v_th=1.0, v_reset=None, detach_reset=True, alpha=2.0):
    """BPTT through the multi-step ParametricLIFNode (sdf_plif_bwd): (dL/dx, dL/dk), dL/dk a one-element fp32 tensor reduced in a
    fixed order (no atomics); ATan surrogate."""
    T, N = x.shape[0], x[0].numel()
    gx = torch.empty_like(x)
    gk = torch.empty((1,), dtype=torch.float32, device=x.device)
    nbytes = lib().sdf_plif_bwd_workspace_bytes(T, N)
    ws = _ws_f32(nbytes, x.device)
    rc = lib().sdf_plif_bwd(_ptr(x, torch.float32), _ptr(k, torch.float32), _ptr(grad_spike, torch.float32), _ptr(gx), _ptr(gk),
                            _ptr(ws), nbytes, T, N, v_th, *_reset(v_reset), 1 if detach_reset else 0, 0, alpha, _stream())
    _check(rc, "sdf_plif_bwd")
    return gx, gk


@_pad4("x", "grad_spike")
def sltt_bwd(x, grad_spike, tau=2.0, v_th=1.0, v_reset=None, alpha=2.0):
    """Online gradient of the multi-step SLTT-LIF (sdf_sltt_bwd): dL/dx with the membrane detached between steps; ATan surrogate."""
    T, N = x.shape[0], x[0].numel()
    gx = torch.empty_like(x)
    rc = lib().sdf_sltt_bwd(_ptr(x, torch.float32), _ptr(grad_spike, torch.float32), _ptr(gx), T, N, tau, v_th, *_reset(v_reset),
                            0, alpha, _stream())
    _check(rc, "sdf_sltt_bwd")
    return gx


@_pad4("x")
def glif_fwd(x, tab, out_dtype=torch.float32):
    """Multi-step GatedLIFNode over dim 0 (sdf_glif_fwd) from v = 0, s = 0; `tab` = [L, Dk, g, R, th, c_0 .. c_{T-1}], 5 + T fp32 in
    DEVICE memory (read by the kernel, never by the host)."""
    if out_dtype not in (torch.float32, torch.uint8):
        raise SdfError(f"spike dtype {out_dtype} unsupported")
    T, N = x.shape[0], x[0].numel()
    if tab.numel() != 5 + T:
        raise SdfError(f"glif_fwd: the gate table has {tab.numel()} entries, T = {T} needs {5 + T}")
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    rc = lib().sdf_glif_fwd(_ptr(x, torch.float32), _ptr(tab, torch.float32), _ptr(out), T, N,
                            SDF_F32 if out_dtype == torch.float32 else SDF_U8, _stream())
    _check(rc, "sdf_glif_fwd")
    return out


@_pad4("x", "grad_spike")
def glif_bwd(x, tab, grad_spike, alpha=2.0):
    """BPTT through the multi-step GatedLIFNode (sdf_glif_bwd): (dL/dx, dL/dtab), dL/dtab 5 + T fp32 reduced in a fixed order (no
    atomics); ATan surrogate."""
    T, N = x.shape[0], x[0].numel()
    if tab.numel() != 5 + T:
        raise SdfError(f"glif_bwd: the gate table has {tab.numel()} entries, T = {T} needs {5 + T}")
    gx = torch.empty_like(x)
    gtab = torch.empty((5 + T,), dtype=torch.float32, device=x.device)
    nbytes = lib().sdf_glif_bwd_workspace_bytes(T, N)
    ws = _ws_f32(nbytes, x.device)
    rc = lib().sdf_glif_bwd(_ptr(x, torch.float32), _ptr(tab, torch.float32), _ptr(grad_spike, torch.float32), _ptr(gx), _ptr(gtab),
                            _ptr(ws), nbytes, T, N, 0, alpha, _stream())
    _check(rc, "sdf_glif_bwd")
    return gx, gtab


@_pad4("x", "grad_spike")
def psn_bwd(x, W, b, grad_spike, alpha=2.0, need_param_grads=True):
    """Backward of the parallel spiking neuron (sdf_psn_bwd): (dL/dx, dL/dW, dL/db); ATan surrogate.
    T <= 10 reduces dW / db in the kernel; larger T takes grad_h from the kernel and one library GEMM."""
    T, N = x.shape[0], x[0].numel()
    gx = torch.empty_like(x)
    fused = need_param_grads and T <= 10
    gW = torch.empty((T, T), dtype=torch.float32, device=x.device) if fused else None
    gb = torch.empty((T,), dtype=torch.float32, device=x.device) if fused else None
    gh = torch.empty_like(x) if (need_param_grads and not fused) else None
    nbytes = lib().sdf_psn_bwd_workspace_bytes(T, N) if fused else 0
    ws = _ws_f32(nbytes, x.device) if fused else None
    rc = lib().sdf_psn_bwd(_ptr(x, torch.float32), _ptr(W.contiguous(), torch.float32), _ptr(b.contiguous().view(-1), torch.float32),
                           _ptr(grad_spike, torch.float32), _ptr(gx), _ptr(gW), _ptr(gb), _ptr(gh), _ptr(ws), nbytes, T, N, 0, alpha,
                           _stream())
    _check(rc, "sdf_psn_bwd")
    if gh is not None:
        gW, gb = gh.view(T, -1) @ x.view(T, -1).t(), gh.view(T, -1).sum(1)
    return gx, gW, gb


def psn_fwd(x, W, b, out_dtype=torch.float32):
    """Parallel spiking neuron over dim 0 of a contiguous tensor (sdf_psn_fwd; any per-step size)."""
    x = x.contiguous()
    T, N = x.shape[0], x[0].numel()
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    rc = lib().sdf_psn_fwd(_ptr(x, torch.float32), _ptr(W.contiguous(), torch.float32), _ptr(b.contiguous().view(-1), torch.float32),
                           _ptr(out), T, N, SDF_F32 if out_dtype == torch.float32 else SDF_U8, _stream())
    _check(rc, "sdf_psn_fwd")
    return out


def split_weight(W, nsplit=3):
    """fp32 weight (N,K) -> 16-bit planes (nsplit,N,K) stored as int16 bit patterns.
    nsplit 1 / 3: bf16 planes (sdf_split_weight_bf16).  nsplit 2: two fp16 planes of scale * W
    (sdf_split_weight_f16x2) with scale the power of two that puts max|W| in [2^14, 2^15); the matching accumulator
    scale 1 / scale travels with the tensor as the attribute `sdf_acc_scale`."""
    W = W.contiguous()
    planes = torch.empty((nsplit,) + tuple(W.shape), dtype=torch.int16, device=W.device)
    if nsplit == 2:
        import math
        mx = float(W.detach().abs().max())
        scale = 2.0 ** (14 - math.floor(math.log2(mx))) if mx > 0 and math.isfinite(mx) else 1.0
        scale = min(max(scale, 2.0 ** -100), 2.0 ** 100)
        _check(lib().sdf_split_weight_f16x2(_ptr(W, torch.float32), planes.data_ptr(), W.numel(), scale, _stream()),
               "sdf_split_weight_f16x2")
        planes.sdf_acc_scale = 1.0 / scale
        return planes
    _check(lib().sdf_split_weight_bf16(_ptr(W, torch.float32), planes.data_ptr(), W.numel(), nsplit, _stream()), "sdf_split_weight_bf16")
    return planes


PLANES_I8X3 = 4
PLANES_I8X3_TILED = 5


def split_weight_i8x3(W):
    """fp32 weight (N, K) -> int8 digit planes (3, N, K) + per-row power-of-two scales (attribute `sdf_col_scale`):
    w = (d2*65536 + d1*256 + d0) * scale (sdf_split_weight_i8x3).  Read by the weight-resident 3x3 convolution and the wide-stage
    kernels of the swin blocks (csrc/ms_wide.hip)."""
    W = W.contiguous()
    N, K = W.shape
    planes = torch.empty((3, N, K), dtype=torch.int8, device=W.device)
    scale = torch.empty((N,), dtype=torch.float32, device=W.device)
    _check(lib().sdf_split_weight_i8x3(_ptr(W, torch.float32), planes.data_ptr(), scale.data_ptr(), N, K, _stream()),
           "sdf_split_weight_i8x3")
    planes.sdf_col_scale = scale
    return planes


def conv_wres_applicable(imgs, H, W, Cin, Cout, stride, T=1):
    """Mirror of the library's dispatch rule (csrc/spike_conv_wres.hip: spike_conv_wres_plan): 3x3 on 96 input channels at
    stride 1 or - digit planes only - at stride 2 on 48 (the patch embedding's first 3x3) or 96 channels (its projection), output columns in blocks of 32, and enough
    8 x 16 pixel OUTPUT tiles (x T steps each when the neuron is fused) to give every half workgroup of the chip work - below that
    the streaming kernels' split-K wins.  H, W: the input image."""
    if sw("SDF_CONV_WRES", "") == "0":             # the library's A/B override: always the streaming kernels (which
        return False                                             # do not read digit planes: the caller must keep its 16-bit planes)
    if (Cin, stride) not in ((96, 1), (48, 2), (96, 2)) or Cout % 32 or ((Cin, stride) == (96, 2) and T != 1):
        return False                                             # (96 channels at stride 2: two channel passes, fp32 epilogue only)
    oh, ow = (H - 1) // stride + 1, (W - 1) // stride + 1
    if imgs * max(oh * ow * Cout * 4, H * W * Cin) >= 1 << 31:   # the kernel addresses its operands with 31-bit byte offsets
        return False
    tiles = (imgs // T) * (-(-oh // 8)) * (-(-ow // 16))
    return tiles * (Cout // 32) >= 512


def wide_conv_applicable(imgs, H, W, Cin, Cout, stride, T):
    """Mirror of the library's dispatch rule for the small-M digit convolution (csrc/ms_wide.hip: wide_conv_plan): 3x3 / stride 1
    on Cin % 128 == 0 channels, at most 131 072 output rows (SDF_WIDE_MAXROWS) in (B, T, H, W) order with T in {10, 20}."""
    if sw("SDF_WIDE", "") == "0" or sw("SDF_WIDE_CONV", "") != "1" or stride != 1 or Cin % 128 or Cout % 32:
        return False                                             # (opt-in: measured no faster than the streaming kernel + split-K, docs/history/DESIGN_rounds1-5.md)
    return T in (10, 20) and imgs % T == 0 and imgs * H * W <= int(sw("SDF_WIDE_MAXROWS", 131072))


def smallm_conv_applicable(imgs, H, W, Cin, Cout, stride, T):
    """Mirror of the library's dispatch rule for the small-M digit convolution (csrc/ms_smallm.hip: smallm_conv_plan): 3x3 / stride 1
    on Cin % 64 == 0 channels, at most 32 000 output rows (SDF_SMALLM_CONV_ROWS; 5 120 until round 5) in (B, T, H, W) order with T in {10, 20}."""
    if sw("SDF_SMALLM", "") == "0" or stride != 1 or Cin % 64 or Cout % 32:
        return False
    return T in (10, 20) and imgs % T == 0 and imgs * H * W <= int(sw("SDF_SMALLM_CONV_ROWS", 400 * 80))


def tile_weight_i8x3(planes):
    """sdf_tile_weight_i8x3: digit planes (3, N, K) -> the same digits in MFMA fragment order [N / 16][K / 64][3][64][16 B] (kept under
    the shape (3, N, K); attribute `sdf_tiled`): what the small-M convolution streams at full rate (csrc/ms_smallm.hip)."""
    _, N, K = planes.shape
    tiled = torch.empty_like(planes)
    _check(lib().sdf_tile_weight_i8x3(_ptr(planes, torch.int8), tiled.data_ptr(), N, K, _stream()), "sdf_tile_weight_i8x3")
    tiled.sdf_col_scale = planes.sdf_col_scale
    tiled.sdf_tiled = True
    return tiled


def smallm_gemm_applicable(M, N, K):
    """Mirror of the library's rule for the plain small-M product (csrc/ms_smallm.hip: smallm_gemm_supports) plus the engine's
    own bound: it pays where K is long enough to amortise a workgroup's prologue and reduction (measured: the first decoder's
    1 080 x 3 456 x 1 536 product; not the second's 4 320 x 1 728 x 832)."""
    if sw("SDF_SMALLM", "") == "0" or M % 10 or N % 32 or K % 64:
        return False
    return M <= 64 * 80 and K >= int(sw("SDF_SMALLM_MINK", 1024))


def smallm_gemm_rows_ok(M):
    """Rows ONE launch of the plain small-M product admits (the library's bound, csrc/ms_smallm.hip smallm_gemm_supports) - wider than the
    routing rule above, which decides per sample: replicas run the product their batch-1 forward takes, in as few launches as this allows."""
    return M % 10 == 0 and M <= int(sw("SDF_SMALLM_CONV_ROWS", 400 * 80))


def res_gemm_applicable(M, N, K):
    """Mirror of the library's rule for the plain product on row-major digit planes (csrc/spike_gemm.hip -> ms_res.hip: whole-K digits
    LDS-resident per 32 columns, row loop): rows in tens, K <= 1024 in steps of 16."""
    if sw("SDF_RES", "") == "0" or sw("SDF_RES_GEMM", "") == "0":
        return False
    return M % 10 == 0 and N % 32 == 0 and K % 16 == 0 and 32 <= K <= 1024 and M * max(K, 4 * N) < 1 << 31


def pack_conv_weight_i8x3(w, tiled=False):
    """Conv2d weight (Cout, Cin, KH, KW) fp32 -> int8 digit planes (3, Cout, KH*KW*Cin), K in (ky, kx, cin) order; `tiled`: in the
    fragment order of tile_weight_i8x3."""
    Cout, Cin, KH, KW = w.shape
    planes = split_weight_i8x3(w.detach().float().permute(0, 2, 3, 1).reshape(Cout, KH * KW * Cin))
    return tile_weight_i8x3(planes) if tiled else planes


def _acc_scale(Wp):
    if Wp.dtype == torch.int8 or Wp.shape[0] != 2:
        return 0.0
    if not hasattr(Wp, "sdf_acc_scale"):
        raise SdfError("fp16 weight planes without their scale: use the tensor returned by split_weight(W, 2) as is")
    return Wp.sdf_acc_scale


def spike_gemm(A, Wp, out, M, N, K, lda=None, ldo=None, bias=None, alpha=None, beta=None, resid=None,
               out_rowmap=None, zg=None):
    """sdf_spike_gemm_fwd.  A: u8 spikes, Wp: int16 (nsplit,N,K) bf16 planes, out: fp32.
    zg = (nH, Tq, B_, N1[, windows per replica]) selects the head-scramble A addressing."""
    d = SpikeGemmDesc()
    d.A, d.Wp, d.out = _ptr(A, torch.uint8), _ptr(Wp), _ptr(out, torch.float32)
    d.M, d.N, d.K = M, N, K
    d.lda = K if lda is None else lda
    d.ldo = N if ldo is None else ldo
    d.nsplit, d.acc_scale = Wp.shape[0], _acc_scale(Wp)
    if Wp.dtype == torch.int8:
        # digit planes: in fragment order (tile_weight_i8x3) the small-M kernel's operand, row-major (split_weight_i8x3) the
        # weight-resident row-loop kernel's (csrc/ms_res.hip: K <= 1024, M % 10 == 0)
        d.nsplit = PLANES_I8X3_TILED if getattr(Wp, "sdf_tiled", False) else PLANES_I8X3
        d.col_scale = _ptr(Wp.sdf_col_scale, torch.float32)
    elif Wp.dtype != torch.int16:
        raise SdfError(f"weight planes must be int16 (16-bit float planes) or int8 (tiled digit planes), got {Wp.dtype}")
    d.bias, d.alpha, d.beta = _ptr(bias, torch.float32), _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    d.resid, d.out_rowmap = _ptr(resid, torch.float32), _ptr(out_rowmap, torch.int32)
    if out_rowmap is not None:
        d.out_rows = out.numel() // d.ldo
    if zg is not None:
        d.zg_nH, d.zg_T, d.zg_B, d.zg_N1 = zg[:4]
        d.zg_rep = zg[4] if len(zg) > 4 else 0                 # (windows per independent replica: SdfSpikeGemmDesc.zg_rep)
    _set_ws(d, A)
    _note(flop=2 * int(d.M) * int(d.N) * int(d.K), shape=(int(d.M), int(d.N), int(d.K)))
    _check(lib().sdf_spike_gemm_fwd(C.byref(d), _stream()), "sdf_spike_gemm_fwd")
    return out


def spike_gemm_sn(A, Wp, out_spike, N, K, T, pos_count, pos_inner, pos_ostride, t_stride, p: NeuronParams,
                  alpha=None, beta=None, add=None, add_prows=0, lda=None):
    """sdf_spike_gemm_fwd with the fused neuron epilogue: out_spike (rows,N) u8 = SN_T(BN(A W^T) [+ add])."""
    d = SpikeGemmDesc()
    d.A, d.Wp, d.out_spike = _ptr(A, torch.uint8), _ptr(Wp, torch.int16), _ptr(out_spike, torch.uint8)
    d.M, d.N, d.K = pos_count * T, N, K
    d.lda, d.ldo, d.nsplit, d.acc_scale = (K if lda is None else lda), N, Wp.shape[0], _acc_scale(Wp)
    d.alpha, d.beta = _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    d.sn_T, d.sn_kind, d.tau, d.v_th = T, KIND[p.kind], p.tau, p.v_th
    d.soft_reset, d.v_reset = _reset(p.v_reset)
    d.psn_w, d.psn_b = _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32)
    d.pos_count, d.pos_inner, d.pos_ostride, d.t_stride = pos_count, pos_inner, pos_ostride, t_stride
    d.add, d.add_prows = _ptr(add, torch.float32), add_prows
    _note(flop=2 * int(d.M) * int(d.N) * int(d.K), shape=(int(d.M), int(d.N), int(d.K)))
    _check(lib().sdf_spike_gemm_fwd(C.byref(d), _stream()), "sdf_spike_gemm_fwd")
    return out_spike


def qk_gate(q, k, e, Tq, rows, Cch, p: NeuronParams, ldq=None, ldk=None):
    """sdf_qk_gate_strided_fwd on u8 spike tensors laid out (Tq, rows, C); q / k rows may be ldq / ldk bytes apart
    (the halves of a fused q|k GEMM output)."""
    soft_reset, v_reset = _reset(p.v_reset)
    rc = lib().sdf_qk_gate_strided_fwd(_ptr(q, torch.uint8), _ptr(k, torch.uint8), _ptr(e, torch.uint8), Tq, rows, Cch,
                                       Cch if ldq is None else ldq, Cch if ldk is None else ldk, KIND[p.kind], p.tau, p.v_th,
                                       v_reset, soft_reset, _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32), _stream())
    _check(rc, "sdf_qk_gate_strided_fwd")
    return e


def qk_gate_glif(q, k, e, Tq, rows, Cch, tab, ldq=None, ldk=None, gate=None):
    """sdf_qk_gate_glif_fwd: qk_gate with a GLIF gate node (`tab` = its 5 + Tq gate table on the device); `gate` (Tq, rows, C / 32) u8
    also receives the gate's own spikes."""
    if tab.numel() != 5 + Tq:
        raise SdfError(f"qk_gate_glif: the gate table has {tab.numel()} entries, T' = {Tq} needs {5 + Tq}")
    if gate is not None and (not gate.is_contiguous() or gate.numel() != Tq * rows * (Cch // 32)):
        raise SdfError("qk_gate_glif: `gate` must be a contiguous (Tq, rows, C / 32) u8 tensor")
    rc = lib().sdf_qk_gate_glif_fwd(_ptr(q, torch.uint8), _ptr(k, torch.uint8), _ptr(e, torch.uint8), _ptr(gate, torch.uint8),
                                    _ptr(tab, torch.float32), Tq, rows, Cch, Cch if ldq is None else ldq, Cch if ldk is None else ldk,
                                    _stream())
    _check(rc, "sdf_qk_gate_glif_fwd")
    return e


SDF_QK_KEEP_SPIKES, SDF_QK_FOUR_LAUNCHES, SDF_QK_NARROW = 1, 2, 4


def _ncfg(c, p: NeuronParams):
    c.kind, c.tau, c.v_th = KIND[p.kind], p.tau, p.v_th
    c.soft_reset, c.v_reset = _reset(p.v_reset)
    c.psn_w, c.psn_b = _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32)


def window_slice_map(B, D, H, W, ws, ss, device):
    """sdf_window_slice_map: the int32 gather table of pad + roll + window_partition_v2, built on the device.
    Returns (map (B_*Wd*Wh*Ww,), B_)."""
    Wd, Wh, Ww = ws
    if torch.device(device).type != "cuda":
        raise SdfError("window_slice_map builds the map on the GPU (no CPU fallback)")
    B_ = B * -(-D // Wd) * -(-H // Wh) * -(-W // Ww)
    m = torch.empty((B_ * Wd * Wh * Ww,), dtype=torch.int32, device=device)
    nw = C.c_int64(0)
    _check(lib().sdf_window_slice_map(m.data_ptr(), B, D, H, W, Wd, Wh, Ww, ss[0], ss[1], ss[2], C.byref(nw), _stream()),
           "sdf_window_slice_map")
    assert nw.value == B_
    return m, B_


def replica_slice_map(map1, nW, R, Tq, N1, x_rows1):
    """The slice map of R INDEPENDENT batch-1 problems from the batch-1 table `map1` ((Tq * nW * N1,) int32, nW windows, x_rows1
    rows of x per sample): entry (t' * R * nW + r * nW + b') * N1 + n = r * x_rows1 + map1[(t' * nW + b') * N1 + n] (-1 stays -1).
    Attention step t' of window b' of replica r is then that replica's own slice t' * nW + b' - the reference's batch-1
    `window_partition_v2` view (Spiking_swin_transformer3D.py:100-113) per sample instead of its batch-coupling view over R samples -
    while the kernels see ONE (Tq, R * nW, N1, C) problem.  Index arithmetic on the device, no kernel."""
    m = map1.view(Tq, 1, nW * N1).expand(Tq, R, nW * N1)
    off = (torch.arange(R, device=map1.device, dtype=torch.int32) * x_rows1).view(1, R, 1)
    return torch.where(m >= 0, m + off, m).reshape(-1).contiguous()


def replica_zsrc_map(z1, nW, R, Tq, N1, Cc):
    """The projection's operand map (window_zsrc_map) of R independent batch-1 problems from the batch-1 table `z1` (int32 per row of
    x: byte offset of the row's gated spikes in the replica's OWN E_flat, a (Tq, nW, N1, C) tensor): that tensor is the sub-block
    [:, r * nW : (r + 1) * nW] of the (Tq, R * nW, N1, C) buffer the kernels share, so offset o of replica r moves to
    ((o // half) * R * nW + r * nW) * N1 * C + o % half with half = nW * N1 * C.  nW % Tq == 0 keeps the nH pieces of a row on one side
    of `half` (the kernels step from head to head by a constant Tq * N1 * 32)."""
    if nW % Tq:
        raise ReplicaGeometryError(f"replicas need a window count per sample ({nW}) that is a multiple of the window depth ({Tq})")
    half = nW * N1 * Cc
    te = z1 // half
    r = torch.arange(R, device=z1.device, dtype=torch.int32).view(R, 1)
    out = (te.view(1, -1) * (R * nW) + r * nW) * (N1 * Cc) + (z1 - te * half).view(1, -1)
    if R * Tq * nW * N1 * Cc >= 1 << 31:
        raise SdfError("replica batch too large for the 31-bit operand offsets of the projection")
    return out.to(torch.int32).reshape(-1).contiguous()


def _digits(dg):
    """(planes pointer, channel-scale pointer) of int8 digit planes made by split_weight_i8x3, or (None, None)."""
    if dg is None:
        return None, None
    return _ptr(dg, torch.int8), _ptr(dg.sdf_col_scale, torch.float32)


def window_zsrc_map(slice_map, B_, Tq, N1, nH, x_rows):
    """sdf_window_zsrc_map: per row of x the byte offset of its gated spikes in E behind the reference's head scramble - what the
    wide-stage projection (csrc/ms_wide.hip) gathers its operand through.  int32 (x_rows,)."""
    z = torch.zeros((x_rows,), dtype=torch.int32, device=slice_map.device)
    _check(lib().sdf_window_zsrc_map(slice_map.data_ptr(), B_, Tq, N1, nH, z.data_ptr(), _stream()), "sdf_window_zsrc_map")
    return z


def qk_attn(x, slice_map, B_, Tq, N1, nH, p_lin, sn_proj, sn_q, sn_k, sn2_q, qk=None, q_lin=None, k_lin=None, pe=None, keep_ws=None,
            four_launches=False, x_src=None, emit=None, narrow=False, info=None, rep_windows=0, ws=None):
    """sdf_qk_attn_fwd: x (B,D,H,W,C) fp32 channel-last += SSA(x), in place.  `qk` = {"Wp", "alpha", "beta", "add"} for the
    stacked projection, or q_lin / k_lin (objects with Wp / alpha / beta) + pe for separate ones; p_lin has Wp / bias / alpha / beta.
    `x_src` (window_zsrc_map) lets the library take its wide-stage kernels; `emit` = (u8 buffer, NeuronParams): the projection
    also writes SN(x after the update) over D there (the MLP's first neuron) when the call runs on the wide-stage kernels - `info`
    (a dict) then receives "emitted": True; `narrow` forces the general kernels (A/B).  `rep_windows` > 0: the B_ windows are
    B_ / rep_windows independent batch-1 problems and `slice_map` / `x_src` their concatenated tables (replica_slice_map, replica_zsrc_map).
    `ws`: the caller's workspace, a 256-byte aligned u8 buffer of at least sdf_qk_attn_workspace_bytes (as ms_mlp's `ws`); default: allocated here."""
    Cc = x.shape[-1]
    d = QkAttnDesc()
    d.rep_windows = rep_windows
    d.x, d.slice_map = _ptr(x, torch.float32), _ptr(slice_map, torch.int32)
    d.B_, d.x_rows, d.Tq, d.N1, d.C, d.nH = B_, x.numel() // Cc, Tq, N1, Cc, nH
    d.nsplit = p_lin.Wp.shape[0]
    if qk is not None:
        d.qk_planes, d.qk_alpha, d.qk_beta = _ptr(qk["Wp"], torch.int16), _ptr(qk["alpha"], torch.float32), _ptr(qk["beta"], torch.float32)
        d.qk_add, d.qk_acc_scale = _ptr(qk["add"], torch.float32), _acc_scale(qk["Wp"])
    else:
        d.q_planes, d.q_alpha, d.q_beta, d.q_acc_scale = _ptr(q_lin.Wp, torch.int16), _ptr(q_lin.alpha), _ptr(q_lin.beta), _acc_scale(q_lin.Wp)
        d.k_planes, d.k_alpha, d.k_beta, d.k_acc_scale = _ptr(k_lin.Wp, torch.int16), _ptr(k_lin.alpha), _ptr(k_lin.beta), _acc_scale(k_lin.Wp)
        d.k_add = _ptr(pe, torch.float32)
    d.p_planes, d.p_bias, d.p_alpha, d.p_beta = _ptr(p_lin.Wp, torch.int16), _ptr(p_lin.bias), _ptr(p_lin.alpha), _ptr(p_lin.beta)
    d.p_acc_scale = _acc_scale(p_lin.Wp)
    for c, p in ((d.sn_proj, sn_proj), (d.sn_q, sn_q), (d.sn_k, sn_k), (d.sn2_q, sn2_q)):
        _ncfg(c, p)
    nbytes = lib().sdf_qk_attn_workspace_bytes(B_, Tq, N1, Cc)
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)      # intermediates: caller-owned, caching allocator
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < nbytes or ws.data_ptr() % 256:
        raise SdfError(f"qk_attn: `ws` must be a contiguous, 256-byte aligned u8 buffer of at least {nbytes} bytes")
    d.workspace, d.workspace_bytes = _ptr(ws, torch.uint8), ws.numel()
    gws = workspace(x.device)
    d.gemm_workspace, d.gemm_workspace_bytes = gws.data_ptr(), gws.numel()
    d.flags = (SDF_QK_KEEP_SPIKES if keep_ws is not None else 0) | (SDF_QK_FOUR_LAUNCHES if four_launches else 0) | \
        (SDF_QK_NARROW if narrow else 0)
    if x_src is not None:
        d.x_src, d.xB, d.xD, d.xHW = _ptr(x_src, torch.int32), x.shape[0], x.shape[1], x.shape[2] * x.shape[3]
        # the wide-stage kernels multiply int8 digit planes (`digits` of the layer objects / of the qk dict, made by split_weight_i8x3)
        d.p_digits, d.p_cscale = _digits(getattr(p_lin, "digits", None))
        if qk is not None:
            d.qk_digits, d.qk_cscale = _digits(qk.get("digits"))
        else:
            d.q_digits, d.q_cscale = _digits(getattr(q_lin, "digits", None))
            d.k_digits, d.k_cscale = _digits(getattr(k_lin, "digits", None))
    if emit is not None:
        # the query sees the descriptor as the call will (emit neuron included: the library refuses neurons it has no epilogue for);
        # refused -> the call runs without the emission and the caller's MLP runs its own first neuron
        d.emit_s1 = _ptr(emit[0], torch.uint8)                # (only the wide-stage projection emits the next neuron's spikes)
        _ncfg(d.emit_sn, emit[1])
        if lib().sdf_qk_attn_is_wide(C.byref(d)) == 1:
            if info is not None:
                info["emitted"] = True
        else:
            d.emit_s1 = None
            _ncfg(d.emit_sn, NeuronParams())
    _note(flop=2 * Tq * B_ * N1 * Cc * 3 * Cc, shape=(Tq * B_ * N1, Cc))
    _check(lib().sdf_qk_attn_fwd(C.byref(d), _stream()), "sdf_qk_attn_fwd")
    if keep_ws is not None:
        keep_ws.append(ws)                  # the call's intermediates (u8 spikes, layout: sdf_qk_attn_workspace_bytes) for the parity tape
    return x


MLP_KEEP_SPIKES, MLP_THREE_LAUNCHES, MLP_NARROW = 1, 2, 4


def ms_mlp_workspace(x, Ch):
    """The caller-owned workspace of ms_mlp for x (B,D,H,W,C): u8, SN1's spikes [tokens][C] at its head (what qk_attn's `emit` fills)."""
    B, D, H, W, Cc = x.shape
    nbytes = lib().sdf_ms_mlp_workspace_bytes(B * D * H * W, Cc, Ch)
    return torch.empty((nbytes,), dtype=torch.uint8, device=x.device)


def ms_mlp(x, fc1, fc2, sn1, sn2, keep_ws=None, three_launches=False, ws=None, s1_ready=False, narrow=False, emit_next=None):
    """sdf_ms_mlp_fwd: x (B,D,H,W,C) fp32 channel-last += MLP(x) over the time axis D, in place.  `keep_ws` (a list) receives
    the workspace with the SN1 / SN2 spikes (parity tape); `three_launches` selects the unfused A/B reference.  `ws` =
    ms_mlp_workspace(...) of the caller; with `s1_ready` its head already holds SN1(x) (wide stages: written by qk_attn's `emit`).
    `emit_next` = (u8 (B,D,H,W,C) buffer, neuron): wide stages only - the last launch also writes that neuron's spikes of the
    updated x (the patch merging's / the bottleneck's first neuron)."""
    B, D, H, W, Cc = x.shape
    d = MsMlpDesc()
    d.x, d.B, d.D, d.HW, d.C, d.Ch, d.nsplit = _ptr(x, torch.float32), B, D, H * W, Cc, fc1.N, fc1.Wp.shape[0]
    d.fc1_planes, d.fc1_alpha, d.fc1_beta, d.fc1_acc_scale = _ptr(fc1.Wp, torch.int16), _ptr(fc1.alpha), _ptr(fc1.beta), _acc_scale(fc1.Wp)
    d.fc2_planes, d.fc2_alpha, d.fc2_beta, d.fc2_acc_scale = _ptr(fc2.Wp, torch.int16), _ptr(fc2.alpha), _ptr(fc2.beta), _acc_scale(fc2.Wp)
    _ncfg(d.sn1, sn1)
    _ncfg(d.sn2, sn2)
    if ws is None:
        if s1_ready:
            raise SdfError("s1_ready needs the caller's workspace (ms_mlp_workspace) with SN1's spikes at its head")
        ws = ms_mlp_workspace(x, fc1.N)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    gws = workspace(x.device)
    d.gemm_workspace, d.gemm_workspace_bytes = gws.data_ptr(), gws.numel()
    d.flags = (MLP_KEEP_SPIKES if keep_ws is not None else 0) | (MLP_THREE_LAUNCHES if three_launches else 0) | (MLP_NARROW if narrow else 0)
    d.fc1_digits, d.fc1_cscale = _digits(getattr(fc1, "digits", None))
    d.fc2_digits, d.fc2_cscale = _digits(getattr(fc2, "digits", None))
    d.fc2_tiled = _ptr(getattr(fc2, "digits_tiled", None), torch.int8)      # (fragment order: fc2 on the small-M kernel, csrc/ms_smallm.hip)
    if s1_ready:
        d.s1_in = ws.data_ptr()
    if emit_next is not None:
        buf, nsn = emit_next
        if buf.numel() != x.numel() or buf.dtype != torch.uint8:
            raise SdfError("emit_next: need a u8 buffer of x's shape")
        d.emit_next = _ptr(buf, torch.uint8)
        _ncfg(d.emit_sn, nsn)
    if (s1_ready or emit_next is not None) and lib().sdf_ms_mlp_is_wide(C.byref(d)) != 1:
        raise SdfError("s1_ready / emit_next: this MLP does not run on the wide-stage kernels (they would be ignored)")
    _note(flop=4 * B * D * H * W * Cc * fc1.N, shape=(B * D * H * W, Cc, fc1.N))
    _check(lib().sdf_ms_mlp_fwd(C.byref(d), _stream()), "sdf_ms_mlp_fwd")
    if keep_ws is not None:
        keep_ws.append(ws)
    return x


def ms_mlp_is_wide(x, fc1, fc2, sn1, sn2, emit_sn=None):
    """Whether ms_mlp of this layer on x runs on the wide-stage kernels (host-only query; then `s1_ready` / `emit_next` - with the
    neuron `emit_sn` - are accepted)."""
    if getattr(fc1, "digits", None) is None or getattr(fc2, "digits", None) is None:
        return False
    B, D, H, W, Cc = x.shape
    d = MsMlpDesc()
    d.x, d.B, d.D, d.HW, d.C, d.Ch, d.nsplit = _ptr(x, torch.float32), B, D, H * W, Cc, fc1.N, fc1.Wp.shape[0]
    d.fc1_planes, d.fc2_planes = _ptr(fc1.Wp, torch.int16), _ptr(fc2.Wp, torch.int16)
    d.fc1_alpha, d.fc1_beta, d.fc2_alpha, d.fc2_beta = _ptr(fc1.alpha), _ptr(fc1.beta), _ptr(fc2.alpha), _ptr(fc2.beta)
    _ncfg(d.sn1, sn1)
    _ncfg(d.sn2, sn2)
    d.workspace, d.workspace_bytes = 256, 1 << 40               # not dereferenced by the query
    if emit_sn is not None:
        d.emit_next = 256
        _ncfg(d.emit_sn, emit_sn)
    d.fc1_digits, d.fc1_cscale = _digits(fc1.digits)
    d.fc2_digits, d.fc2_cscale = _digits(fc2.digits)
    return lib().sdf_ms_mlp_is_wide(C.byref(d)) == 1


def ms_patch_merge(spikes, lin, out=None):
    """sdf_ms_patch_merge_fwd: spikes u8 (B,D,H,W,C) = SN(x) -> BN(cat_2x2(spikes) W^T) fp32 (B,D,ceil(H/2),ceil(W/2),N); `lin` carries
    the reduction weight as digit planes (`digits`) and the BatchNorm as (alpha, beta).  Returns None when the shape is not covered
    (the caller keeps its gather map + spike_gemm)."""
    B, D, H, W, Cc = spikes.shape
    if getattr(lin, "digits", None) is None:
        return None
    d = MsMergeDesc()
    d.spikes = _ptr(spikes, torch.uint8)
    d.digits, d.cscale = _digits(lin.digits)
    d.alpha, d.beta = _ptr(lin.alpha), _ptr(lin.beta)
    d.B, d.D, d.H, d.W, d.C, d.N = B, D, H, W, Cc, lin.N
    if out is None:
        out = torch.empty((B, D, (H + 1) // 2, (W + 1) // 2, lin.N), dtype=torch.float32, device=spikes.device)
    d.out = _ptr(out, torch.float32)
    _note(flop=2 * out.numel() * 4 * Cc, shape=(out.numel() // lin.N, lin.N, 4 * Cc))
    rc = lib().sdf_ms_patch_merge_fwd(C.byref(d), _stream())
    if rc == E_SHAPE:
        return None
    _check(rc, "sdf_ms_patch_merge_fwd")
    return out


def bn_train_fwd(x2, weight, bias, running_mean, running_var, momentum, eps):
    """sdf_bn_train_fwd on a contiguous (R, C) fp32 buffer: (y, save_mean, save_invstd); running stats updated in place."""
    R, Cc = x2.shape
    y = torch.empty_like(x2)
    mean, invstd = torch.empty(Cc, dtype=torch.float32, device=x2.device), torch.empty(Cc, dtype=torch.float32, device=x2.device)
    nbytes = lib().sdf_bn_train_workspace_bytes(R, Cc)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x2.device)
    rc = lib().sdf_bn_train_fwd(_ptr(x2, torch.float32), _ptr(weight, torch.float32), _ptr(bias, torch.float32), _ptr(y), _ptr(mean),
                                _ptr(invstd), _ptr(running_mean, torch.float32), _ptr(running_var, torch.float32), R, Cc, eps, momentum,
                                ws.data_ptr(), nbytes, _stream())
    _check(rc, "sdf_bn_train_fwd")
    return y, mean, invstd


def bn_train_bwd(x2, grad_y, weight, mean, invstd):
    """sdf_bn_train_bwd: (grad_x, grad_weight, grad_bias)."""
    R, Cc = x2.shape
    gx = torch.empty_like(x2)
    gw, gb = torch.empty(Cc, dtype=torch.float32, device=x2.device), torch.empty(Cc, dtype=torch.float32, device=x2.device)
    nbytes = lib().sdf_bn_train_workspace_bytes(R, Cc)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x2.device)
    rc = lib().sdf_bn_train_bwd(_ptr(x2, torch.float32), _ptr(grad_y, torch.float32), _ptr(weight, torch.float32), _ptr(mean),
                                _ptr(invstd), _ptr(gx), _ptr(gw), _ptr(gb), R, Cc, ws.data_ptr(), nbytes, _stream())
    _check(rc, "sdf_bn_train_bwd")
    return gx, gw, gb


def bn_train_nchw_supported(x):
    return x.dim() == 4 and (x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[1] <= 2048


def bn_train_nchw_fwd(x, weight, bias, running_mean, running_var, momentum, eps):
    """sdf_bn_train_nchw_fwd on a contiguous (N, C, H, W) fp32 buffer: (y, save_mean, save_invstd)."""
    N, Cc, H, W = x.shape
    y = torch.empty_like(x)
    mean, invstd = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    nbytes = lib().sdf_bn_train_workspace_bytes(N * H * W, (Cc + 3) // 4 * 4)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    rc = lib().sdf_bn_train_nchw_fwd(_ptr(x, torch.float32), _ptr(weight, torch.float32), _ptr(bias, torch.float32), _ptr(y),
                                     _ptr(mean), _ptr(invstd), _ptr(running_mean, torch.float32), _ptr(running_var, torch.float32),
                                     N, Cc, H * W, eps, momentum, ws.data_ptr(), nbytes, _stream())
    _check(rc, "sdf_bn_train_nchw_fwd")
    return y, mean, invstd


def bn_train_nchw_bwd(x, grad_y, weight, mean, invstd):
    N, Cc, H, W = x.shape
    gx = torch.empty_like(x)
    gw, gb = torch.empty(Cc, dtype=torch.float32, device=x.device), torch.empty(Cc, dtype=torch.float32, device=x.device)
    nbytes = lib().sdf_bn_train_workspace_bytes(N * H * W, (Cc + 3) // 4 * 4)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    rc = lib().sdf_bn_train_nchw_bwd(_ptr(x, torch.float32), _ptr(grad_y, torch.float32), _ptr(weight, torch.float32), _ptr(mean),
                                     _ptr(invstd), _ptr(gx), _ptr(gw), _ptr(gb), N, Cc, H * W, ws.data_ptr(), nbytes, _stream())
    _check(rc, "sdf_bn_train_nchw_bwd")
    return gx, gw, gb


def rows_gather(x2, row_map):
    """sdf_rows_gather_fwd: (rows, C) fp32 -> (len(map), C), zero rows where the map is negative."""
    out = torch.empty((row_map.numel(), x2.shape[1]), dtype=torch.float32, device=x2.device)
    _check(lib().sdf_rows_gather_fwd(_ptr(x2, torch.float32), _ptr(row_map, torch.int32), _ptr(out),
                                     row_map.numel(), x2.shape[1], _stream()), "sdf_rows_gather_fwd")
    return out


def rows_scatter(y2, row_map, rows):
    """sdf_rows_scatter_fwd: (len(map), C) fp32 -> (rows, C): out[map[i]] = y2[i]; rows nobody names are zero."""
    out = torch.zeros((rows, y2.shape[1]), dtype=torch.float32, device=y2.device)
    _check(lib().sdf_rows_scatter_fwd(_ptr(y2, torch.float32), _ptr(row_map, torch.int32), _ptr(out),
                                      row_map.numel(), y2.shape[1], _stream()), "sdf_rows_scatter_fwd")
    return out


def qk_gate_f32(q, k, p: NeuronParams):
    """sdf_qk_gate_f32_fwd: e = k * SN2_q(head sums of q) on fp32 spike tensors (Tq, rows, C) (training path)."""
    q, k = q.contiguous(), k.contiguous()
    Tq, Cc = q.shape[0], q.shape[-1]
    e = torch.empty_like(k)
    rc = lib().sdf_qk_gate_f32_fwd(_ptr(q, torch.float32), _ptr(k, torch.float32), _ptr(e), Tq, q[0].numel() // Cc, Cc, KIND[p.kind],
                                   p.tau, p.v_th, *_reset(p.v_reset), _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32), _stream())
    _check(rc, "sdf_qk_gate_f32_fwd")
    return e


def qk_gate_bwd(q, k, grad_e, p: NeuronParams, detach_reset=True, alpha=2.0):
    """sdf_qk_gate_bwd: (dL/dq, dL/dk, dL/dW, dL/db) of the token gate (the last two only for a PSN gate, else None)."""
    q, k, g = q.contiguous(), k.contiguous(), grad_e.contiguous()
    Tq, Cc = q.shape[0], q.shape[-1]
    rows = q[0].numel() // Cc
    gq, gk = torch.empty_like(q), torch.empty_like(k)
    psn = p.kind == "psn"
    gW = torch.empty((Tq, Tq), dtype=torch.float32, device=q.device) if psn else None
    gb = torch.empty((Tq,), dtype=torch.float32, device=q.device) if psn else None
    nbytes = lib().sdf_qk_gate_bwd_workspace_bytes(Tq, rows, Cc) if psn else 0
    ws = _ws_f32(nbytes, q.device) if psn else None
    rc = lib().sdf_qk_gate_bwd(_ptr(q, torch.float32), _ptr(k, torch.float32), _ptr(g, torch.float32), _ptr(gq), _ptr(gk), Tq, rows, Cc,
                               KIND[p.kind], p.tau, p.v_th, *_reset(p.v_reset), 1 if detach_reset else 0, 0, alpha,
                               _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32), _ptr(gW), _ptr(gb), _ptr(ws), nbytes, _stream())
    _check(rc, "sdf_qk_gate_bwd")
    return gq, gk, gW, gb


def qk_gate_plif_f32(q, k, plif_k, v_th=1.0, v_reset=None):
    """sdf_qk_gate_plif_f32_fwd: the token gate with a PLIF SN2_q; `plif_k` = sigmoid(w), a one-element fp32 device tensor."""
    q, k = q.contiguous(), k.contiguous()
    Tq, Cc = q.shape[0], q.shape[-1]
    e = torch.empty_like(k)
    rc = lib().sdf_qk_gate_plif_f32_fwd(_ptr(q, torch.float32), _ptr(k, torch.float32), _ptr(e), _ptr(plif_k, torch.float32), Tq,
                                        q[0].numel() // Cc, Cc, v_th, *_reset(v_reset), _stream())
    _check(rc, "sdf_qk_gate_plif_f32_fwd")
    return e


def qk_gate_plif_bwd(q, k, grad_e, plif_k, v_th=1.0, v_reset=None, detach_reset=True, alpha=2.0):
    """sdf_qk_gate_plif_bwd: (dL/dq, dL/dk, dL/d plif_k) of the PLIF token gate; the last one-element, fixed-order reduced."""
    q, k, g = q.contiguous(), k.contiguous(), grad_e.contiguous()
    Tq, Cc = q.shape[0], q.shape[-1]
    rows = q[0].numel() // Cc
    gq, gk = torch.empty_like(q), torch.empty_like(k)
    gpk = torch.empty((1,), dtype=torch.float32, device=q.device)
    nbytes = lib().sdf_qk_gate_plif_bwd_workspace_bytes(Tq, rows, Cc)
    ws = _ws_f32(nbytes, q.device)
    rc = lib().sdf_qk_gate_plif_bwd(_ptr(q, torch.float32), _ptr(k, torch.float32), _ptr(g, torch.float32), _ptr(gq), _ptr(gk),
                                    _ptr(plif_k, torch.float32), _ptr(gpk), _ptr(ws), nbytes, Tq, rows, Cc, v_th, *_reset(v_reset),
                                    1 if detach_reset else 0, 0, alpha, _stream())
    _check(rc, "sdf_qk_gate_plif_bwd")
    return gq, gk, gpk


def affine_resid(x, alpha, beta, Cch, inner, resid=None, out=None):
    """out = fmaf(x, alpha[c], beta[c]) (+ resid) with c = (i // inner) % C (sdf_affine_resid_fwd)."""
    if out is None:
        out = torch.empty_like(x)
    rc = lib().sdf_affine_resid_fwd(_ptr(x, torch.float32), _ptr(alpha, torch.float32), _ptr(beta, torch.float32),
                                    _ptr(resid, torch.float32), _ptr(out, torch.float32), x.numel(), Cch, inner, _stream())
    _check(rc, "sdf_affine_resid_fwd")
    return out


ATTN_BWD_MAX_N = 192          # tokens per window the attention backward kernels stage in LDS (sdf_win_attn_ann_bwd / _sew_bwd)
ATTN_BWD_LARGE_MAX_N = 1024   # ... and the key-blocked ones serve beyond (sdf_win_attn_large_ann_bwd / _sew_bwd), at switch value 2


def check_attn_bwd_window(N, switch):
    """Training at a window the HIP attention backward does not serve is refused before any kernel runs (the forward would succeed on
    sdf_win_attn_large_fwd and `backward` would fail); `switch` = SDF_ANN_ATTN_BWD / SDF_SEW_ATTN_BWD, whose value 0 selects the
    torch composition of the attention, which trains at any window, and whose value 2 opts in to the key-blocked HIP backward
    (csrc/win_attn_large_bwd.hip), which trains at every window up to 1024 tokens."""
    value = sw(switch, "1")
    if value == "2":
        if N > ATTN_BWD_LARGE_MAX_N:
            raise NotImplementedError(f"training with {N}-token windows: the HIP window-attention kernels serve at most {ATTN_BWD_LARGE_MAX_N} "
                                      f"tokens per window; set {switch}=0 to train on the torch composition of the attention instead")
    elif N > ATTN_BWD_MAX_N and value != "0":
        raise NotImplementedError(f"training with {N}-token windows: the HIP window-attention backward serves at most {ATTN_BWD_MAX_N} tokens "
                                  f"per window; set {switch}=0 to train on the torch composition of the attention instead, or {switch}=2 "
                                  f"for the key-blocked HIP backward (up to {ATTN_BWD_LARGE_MAX_N} tokens)")


def _win_attn_fwd(d):
    """The forward entry point by window size: sdf_win_attn_fwd up to 192 tokens, sdf_win_attn_large_fwd beyond (which refuses more
    than 1024 with the library's code)."""
    name = "sdf_win_attn_fwd" if d.N <= 192 else "sdf_win_attn_large_fwd"
    _check(getattr(lib(), name)(C.byref(d), _stream()), name)


def win_attn_ann_windowed(qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH):
    """The same with the window partition / reverse INSIDE the kernel: qkv (rows, 3C) fp32 in the activation's own row order,
    row_map (B_*N,) int32 from `window_slice_map` (pad + roll + partition; -1 = padding token, which reads `pad_qkv` (3C) and
    writes nothing) -> (rows, C) in the activation's row order (window reverse + roll back + crop), untouched rows zero."""
    rows, C3 = qkv.shape
    out = torch.zeros((rows, C3 // 3), dtype=torch.float32, device=qkv.device)
    d = WinAttnDesc()
    d.mode, d.q, d.k, d.v, d.out = 0, _ptr(qkv, torch.float32), _ptr(qkv), _ptr(qkv), _ptr(out)
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, N, C3 // 3 // nH
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    d.row_map, d.pad_qkv = _ptr(row_map, torch.int32), _ptr(pad_qkv, torch.float32)
    _win_attn_fwd(d)
    return out


def _win_attn_ann_bwd(entry, qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH, dout):
    """`win_attn_ann_bwd` / `win_attn_ann_bwd_large` on their entry point (same descriptor, `<entry>_workspace_bytes` beside it)."""
    rows, C3 = qkv.shape
    dev = qkv.device
    dqkv = torch.empty_like(qkv)                                 # every real row lies in exactly one window: all of it is written
    d_pad = torch.empty((C3,), dtype=torch.float32, device=dev)
    d_scale = torch.empty((nH,), dtype=torch.float32, device=dev)
    d_bias = torch.empty((nH, N, N), dtype=torch.float32, device=dev)
    nbytes = getattr(lib(), entry + "_workspace_bytes")(B_, nH, N)
    ws = torch.empty((max(nbytes, 256) // 4,), dtype=torch.float32, device=dev)
    d = WinAttnBwdDesc()
    d.qkv, d.row_map, d.pad_qkv = _ptr(qkv, torch.float32), _ptr(row_map, torch.int32), _ptr(pad_qkv, torch.float32)
    d.dout = _ptr(dout, torch.float32)
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    d.dqkv, d.d_pad, d.d_scale, d.d_bias = _ptr(dqkv), _ptr(d_pad), _ptr(d_scale), _ptr(d_bias)
    d.workspace, d.workspace_bytes = _ptr(ws), nbytes
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, N, C3 // 3 // nH
    _check(getattr(lib(), entry)(C.byref(d), _stream()), entry)
    return dqkv, d_pad, d_scale, d_bias


def win_attn_ann_bwd(qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH, dout):
    """Backward of `win_attn_ann_windowed` (sdf_win_attn_ann_bwd): qkv (rows, 3C), row_map (B_*N,) int32, pad_qkv (3C), scale (nH),
    bias (nH, N, N), mask (nW, N, N) or None as the forward took them; dout = dL/d(output) (rows, C).  -> (dqkv (rows, 3C), d_pad (3C), d_scale (nH), d_bias (nH, N, N)); deterministic (fixed-order window sums)."""
    return _win_attn_ann_bwd("sdf_win_attn_ann_bwd", qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH, dout)


def win_attn_ann_bwd_large(qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH, dout):
    """The same for windows of 193 .. 1024 tokens (sdf_win_attn_large_ann_bwd, csrc/win_attn_large_bwd.hip: keys and queries walked
    in blocks, no (B_, nH, N, N) buffer): arguments and returns of `win_attn_ann_bwd`."""
    return _win_attn_ann_bwd("sdf_win_attn_large_ann_bwd", qkv, row_map, B_, N, pad_qkv, scale, bias, mask, nH, dout)


def ann_attn_block_supported(Cc, nH, N):
    """Mirror of sdf_ann_attn_block_supported: the one-launch attention half block is built for C = 96, three heads, windows of 162.
    SDF_ANN_BLOCK=0 (A/B) and SDF_DENSE_LINEAR=0 (library GEMMs for every Linear, the two inside this kernel included) select the
    four-launch path."""
    return (Cc, nH, N) == (96, 3, 162) and sw("SDF_ANN_BLOCK", "1") != "0" and sw("SDF_DENSE_LINEAR", "1") != "0"


def pack_ann_attn_block_weights(wqkv, wproj, nH):
    """fp16 hi / lo planes of the qkv weight (3C, C) as it stands and of the projection weight (C, C) with the 32 input channels of
    every head in the kernel's accumulator order (include/sdformerflow_hip.h: SdfAnnAttnBlockDesc) -> (planes (2,3C,C), planes (2,C,C))."""
    def planes(w):
        w = w.detach().float()
        hi = w.half()
        return torch.stack([hi, (w - hi.float()).half()]).contiguous()
    Cc = wproj.shape[0]
    j = torch.arange(32)
    a, i = j // 8, j % 8
    perm = torch.where(i < 4, 4 * a + i, 16 + 4 * a + i - 4)
    idx = (torch.arange(nH)[:, None] * 32 + perm[None, :]).reshape(-1).to(wproj.device)
    return planes(wqkv), planes(wproj.detach()[:, idx])


def _hi_lo_planes(w):
    w = w.detach().float()
    hi = w.half()
    return torch.stack([hi, (w - hi.float()).half()]).contiguous()


def _acc_order(n32, device):
    """Column permutation of n32 groups of 32 channels into the order the 16 x 16 MFMA accumulators of two neighbouring tiles leave them."""
    j = torch.arange(32)
    a, i = j // 8, j % 8
    perm = torch.where(i < 4, 4 * a + i, 16 + 4 * a + i - 4)
    return (torch.arange(n32)[:, None] * 32 + perm[None, :]).reshape(-1).to(device)


def ann_mlp_block_supported(Cc, Ch):
    """Mirror of sdf_ann_mlp_block_supported: the one-launch MLP half block is built for C = 96, hidden 384.  SDF_ANN_MLP=0 (A/B) and
    SDF_DENSE_LINEAR=0 (library GEMMs for every Linear) select the three-launch path."""
    return (Cc, Ch) == (96, 384) and sw("SDF_ANN_MLP", "1") != "0" and sw("SDF_DENSE_LINEAR", "1") != "0"


def pack_ann_mlp_block_weights(w1, w2):
    """fp16 hi / lo planes of fc1's weight (Ch, C) as it stands and of fc2's weight (C, Ch) with the hidden channels in the kernel's
    accumulator order (include/sdformerflow_hip.h: SdfAnnMlpBlockDesc) -> (planes (2, Ch, C), planes (2, C, Ch))."""
    return _hi_lo_planes(w1), _hi_lo_planes(w2.detach()[:, _acc_order(w2.shape[1] // 32, w2.device)])


def ann_mlp_block(x, out, ln_w, ln_b, ln_eps, w1_planes, b1, w2_planes, b2):
    """sdf_ann_mlp_block_fwd: out = x + fc2(gelu(fc1(LayerNorm(x)))) on rows x (rows, C) fp32, one launch (reference
    swin_transformer3D_v2.py:312-336).  out may be x."""
    rows, Cc = x.shape
    d = AnnMlpBlockDesc()
    d.x, d.out, d.rows, d.C, d.Ch = _ptr(x, torch.float32), _ptr(out, torch.float32), rows, Cc, w1_planes.shape[1]
    d.ln_w, d.ln_b, d.ln_eps = _ptr(ln_w, torch.float32), _ptr(ln_b, torch.float32), float(ln_eps)
    d.w1, d.b1, d.w2, d.b2 = _ptr(w1_planes, torch.float16), _ptr(b1, torch.float32), _ptr(w2_planes, torch.float16), _ptr(b2, torch.float32)
    _check(lib().sdf_ann_mlp_block_fwd(C.byref(d), _stream()), "sdf_ann_mlp_block_fwd")
    return out


LOG2E = 1.4426950408889634


def ann_attn_block_table(scale, bias, mask):
    """(logit scale * log2 e (nH,), ((bias[h] + mask[w]) * log2 e) (nW, nH, N, N)) - what sdf_ann_attn_block_fwd reads: the softmax runs
    in the log2 domain and the additions of the score are the matrix pipe's accumulator input.  Once per parameter version / mask."""
    t = bias[None] if mask is None else bias[None] + mask[:, None]
    return (scale * LOG2E).contiguous(), (t * LOG2E).contiguous()


def ann_attn_block(x, out, row_map, B_, N, nH, ln_w, ln_b, ln_eps, wqkv_planes, qkv_bias, scale2, table, wproj_planes, proj_bias):
    """sdf_ann_attn_block_fwd: out = x + proj(window attention(LayerNorm(x))) on rows x (rows, C) fp32 through the slice map, one launch
    (reference swin_transformer3D_v2.py:272-310 + :331).  (scale2, table) = ann_attn_block_table(...).  out may be x."""
    rows, Cc = x.shape
    d = AnnAttnBlockDesc()
    d.x, d.out, d.row_map = _ptr(x, torch.float32), _ptr(out, torch.float32), _ptr(row_map, torch.int32)
    d.B_, d.nW, d.nH, d.N, d.C, d.rows = B_, table.shape[0], nH, N, Cc, rows
    d.ln_w, d.ln_b, d.ln_eps = _ptr(ln_w, torch.float32), _ptr(ln_b, torch.float32), float(ln_eps)
    d.wqkv, d.qkv_bias = _ptr(wqkv_planes, torch.float16), _ptr(qkv_bias, torch.float32)
    d.scale, d.table = _ptr(scale2, torch.float32), _ptr(table, torch.float32)
    d.wproj, d.proj_bias = _ptr(wproj_planes, torch.float16), _ptr(proj_bias, torch.float32)
    _check(lib().sdf_ann_attn_block_fwd(C.byref(d), _stream()), "sdf_ann_attn_block_fwd")
    return out


def win_attn_ann(qkv, scale, bias, mask, nH):
    """Fused cosine window attention (sdf_win_attn_fwd, SDF_ATTN_ANN): qkv (B_,N,3C) fp32 -> (B_,N,C)."""
    B_, N, C3 = qkv.shape
    out = torch.empty((B_, N, C3 // 3), dtype=torch.float32, device=qkv.device)
    d = WinAttnDesc()
    d.mode, d.q, d.k, d.v, d.out = 0, _ptr(qkv, torch.float32), _ptr(qkv), _ptr(qkv), _ptr(out)
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, N, C3 // 3 // nH
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    _win_attn_fwd(d)
    return out


def win_attn_sew(q, k, v, scale, bias, mask, nH, Tq, B_, N1):
    """Fused spiking window attention without softmax (SDF_ATTN_SEW): q,k,v u8 (T',B_,N1,C) -> fp32 (T',B_,N1,C)."""
    Cc = q.shape[-1]
    out = torch.empty((Tq, B_, N1, Cc), dtype=torch.float32, device=q.device)
    d = WinAttnDesc()
    d.mode, d.q, d.k, d.v, d.out = 1, _ptr(q, torch.uint8), _ptr(k, torch.uint8), _ptr(v, torch.uint8), _ptr(out)
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, Tq * N1, Cc // nH
    d.Tq, d.N1 = Tq, N1
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    _win_attn_fwd(d)
    return out


def _win_attn_scores(d, device):
    """The attention map of the descriptor's attention (sdf_win_attn_scores_fwd: one kernel for 1 .. 1024 tokens per window, more
    are refused with the library's code) -> (B_, nH, N, N) fp32, window-major."""
    scores = torch.empty((d.B_, d.nH, d.N, d.N), dtype=torch.float32, device=device)
    _check(lib().sdf_win_attn_scores_fwd(C.byref(d), _ptr(scores), _stream()), "sdf_win_attn_scores_fwd")
    return scores


def win_attn_ann_scores(qkv, scale, bias, mask, nH, row_map=None, B_=None, N=None, pad_qkv=None):
    """The softmax probabilities `win_attn_ann` / `win_attn_ann_windowed` multiply v with, which they never store (SDF_ATTN_ANN of
    sdf_win_attn_scores_fwd): qkv (B_,N,3C) fp32, or with `row_map` (B_*N,) int32 qkv (rows, 3C), B_, N and pad_qkv (3C) as
    `win_attn_ann_windowed` takes them (a padding token is a row and a column of the map) -> (B_, nH, N, N) fp32."""
    if row_map is None:
        B_, N = qkv.shape[:2]
    C3 = qkv.shape[-1]
    d = WinAttnDesc()
    d.mode, d.q = 0, _ptr(qkv, torch.float32)
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, N, C3 // 3 // nH
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    if row_map is not None:
        d.row_map, d.pad_qkv = _ptr(row_map, torch.int32), _ptr(pad_qkv, torch.float32)
    return _win_attn_scores(d, qkv.device)


def win_attn_sew_scores(q, k, scale, bias, mask, nH, Tq, B_, N1):
    """The score matrix `win_attn_sew` multiplies v with (SDF_ATTN_SEW of sdf_win_attn_scores_fwd, no softmax): q, k u8
    (T',B_,N1,C) -> (B_, nH, N, N) fp32 on the reference's raw head view, N = T' * N1."""
    Cc = q.shape[-1]
    d = WinAttnDesc()
    d.mode, d.q, d.k = 1, _ptr(q, torch.uint8), _ptr(k, torch.uint8)
    d.B_, d.nW, d.nH, d.N, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, Tq * N1, Cc // nH
    d.Tq, d.N1 = Tq, N1
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    return _win_attn_scores(d, q.device)


def _win_attn_sew_bwd(entry, q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout):
    """`win_attn_sew_bwd` / `win_attn_sew_bwd_large` on their entry point (same descriptor, `<entry>_workspace_bytes` beside it)."""
    Cc, N = q.shape[-1], Tq * N1
    dev = q.device
    dq, dk, dv = (torch.empty((Tq, B_, N1, Cc), dtype=torch.float32, device=dev) for _ in range(3))
    d_bias = torch.empty((nH, N, N), dtype=torch.float32, device=dev)
    nbytes = getattr(lib(), entry + "_workspace_bytes")(B_, nH, N)
    ws = torch.empty((max(nbytes, 256) // 4,), dtype=torch.float32, device=dev)
    d = WinAttnSewBwdDesc()
    d.q, d.k, d.v, d.dout = _ptr(q, torch.uint8), _ptr(k, torch.uint8), _ptr(v, torch.uint8), _ptr(dout, torch.float32)
    d.scale, d.bias, d.mask = _ptr(scale, torch.float32), _ptr(bias, torch.float32), _ptr(mask, torch.float32)
    d.dq, d.dk, d.dv, d.d_bias = _ptr(dq), _ptr(dk), _ptr(dv), _ptr(d_bias)
    d.workspace, d.workspace_bytes = _ptr(ws), nbytes
    d.B_, d.nW, d.nH, d.Tq, d.N1, d.hd = B_, (mask.shape[0] if mask is not None else 1), nH, Tq, N1, Cc // nH
    _check(getattr(lib(), entry)(C.byref(d), _stream()), entry)
    return dq, dk, dv, d_bias


def win_attn_sew_bwd(q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout):
    """Backward of `win_attn_sew` (sdf_win_attn_sew_bwd): q, k, v u8 (T',B_,N1,C), scale (nH), bias (nH,N,N), mask (nW,N,N) or None as
    the forward took them; dout = dL/d(output) (T',B_,N1,C) fp32.  -> (dq, dk, dv (T',B_,N1,C) fp32, d_bias (nH,N,N)); deterministic
    (fixed-order split-K sum over windows for d_bias)."""
    return _win_attn_sew_bwd("sdf_win_attn_sew_bwd", q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout)


def win_attn_sew_bwd_large(q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout):
    """The same for windows of 193 .. 1024 tokens (sdf_win_attn_large_sew_bwd, csrc/win_attn_large_bwd.hip: token blocks streamed
    through LDS): arguments and returns of `win_attn_sew_bwd`."""
    return _win_attn_sew_bwd("sdf_win_attn_large_sew_bwd", q, k, v, scale, bias, mask, nH, Tq, B_, N1, dout)


# ---- dense 3x3 convolution of real-valued activations (ANN patch embedding; csrc/dense_conv_wres.hip) ----
def pack_planes(x):
    """(imgs, C, H, W) fp32 -> activation planes (imgs, ceil(C/16), H, W, 32) fp16: per pixel and 16 channels four pieces of
    {4 x hi, 4 x lo}, value = hi + lo (sdf_pack_planes)."""
    x = x.contiguous()
    imgs, Cc, H, W = x.shape
    planes = torch.empty((imgs, -(-Cc // 16), H, W, 32), dtype=torch.float16, device=x.device)
    _check(lib().sdf_pack_planes(_ptr(x, torch.float32), planes.data_ptr(), imgs, Cc, H, W, _stream()), "sdf_pack_planes")
    return planes


def unpack_planes(planes, Cc):
    """activation planes -> (imgs, Cc, H, W) fp32 (sdf_unpack_planes)."""
    imgs, nch, H, W, _ = planes.shape
    x = torch.empty((imgs, Cc, H, W), dtype=torch.float32, device=planes.device)
    _check(lib().sdf_unpack_planes(_ptr(planes, torch.float16), x.data_ptr(), imgs, Cc, H, W, _stream()), "sdf_unpack_planes")
    return x


def pack_planes_up2(x, planes=None, rec0=0):
    """Bilinear x2 upsampling (F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)) of x (imgs, C, h, w) fp32 - any
    strides, e.g. a channels-last view - straight into activation planes at twice the size; with `planes` / `rec0` it fills records
    rec0 .. of an existing (imgs, R, 2h, 2w, 32) tensor, which is how a channel concatenation is assembled (sdf_pack_planes_up2)."""
    imgs, Cc, h, w = x.shape
    if planes is None:
        planes = torch.empty((imgs, -(-Cc // 16), 2 * h, 2 * w, 32), dtype=torch.float16, device=x.device)
    if tuple(planes.shape[2:]) != (2 * h, 2 * w, 32) or planes.shape[0] != imgs or not planes.is_contiguous():
        raise SdfError("planes must be a contiguous (imgs, R, 2h, 2w, 32) tensor")
    sn, sc, sh, sw = x.stride()
    _check(lib().sdf_pack_planes_up2(_ptr(x, torch.float32), _ptr(planes, torch.float16), imgs, Cc, h, w, sn, sc, sh, sw, rec0,
                                     planes.shape[1], _stream()), "sdf_pack_planes_up2")
    return planes


def pack_planes_zero_up2(x, planes, rec0=0):
    """Zero insertion x2 of x (imgs, C, h, w) fp32 - any strides - into records rec0 .. of the planes tensor (imgs, R, 2h, 2w, 32): output
    pixel (2k, 2l) = x[k, l], every other pixel 0 (sdf_pack_planes_zero_up2): the input of a stride-2 transposed convolution as a stride-1
    correlation, without the zero-filled fp32 image."""
    imgs, Cc, h, w = x.shape
    if tuple(planes.shape[2:]) != (2 * h, 2 * w, 32) or planes.shape[0] != imgs or not planes.is_contiguous():
        raise SdfError("planes must be a contiguous (imgs, R, 2h, 2w, 32) tensor")
    sn, sc, sh, sw_ = x.stride()
    _check(lib().sdf_pack_planes_zero_up2(_ptr(x, torch.float32), _ptr(planes, torch.float16), imgs, Cc, h, w, sn, sc, sh, sw_, rec0,
                                          planes.shape[1], _stream()), "sdf_pack_planes_zero_up2")
    return planes


def pack_dense_conv_weight(w):
    """Conv2d weight (Cout, Cin, 3, 3) fp32 -> fp16 planes (2, Cout, 9 * 16 * ceil(Cin/16)), w = plane0 + plane1, K ordered
    (16-channel record, ky, kx, channel in record); channels beyond Cin are zero."""
    Cout, Cin, KH, KW = w.shape
    if (KH, KW) != (3, 3):
        raise SdfError("dense_conv3x3 takes 3x3 kernels")
    rec = -(-Cin // 16)
    wp = torch.zeros((Cout, rec * 16, 3, 3), dtype=torch.float32, device=w.device)
    wp[:, :Cin] = w.detach().float()
    wk = wp.view(Cout, rec, 16, 3, 3).permute(0, 1, 3, 4, 2).reshape(Cout, rec * 144)
    return _f16_planes(wk)


def dense_conv_slices(records):
    """Record ranges [(first, count)] a convolution over `records` input records is chained from: sixes, then at most one single."""
    six, one = divmod(records, 6)
    if one > 1:
        return None
    return [(6 * i, 6) for i in range(six)] + ([(6 * six, 1)] if one else [])


def dense_conv3x3_wide(xp, wslices, beta=None, relu=False, out_f32=False, out=None):
    """3x3 convolution over any record count `dense_conv_slices` can cut: link k multiplies records [first, first + count) with its own
    weight planes and adds the previous link's result (`resid`); the last link adds beta, applies relu and picks the output format
    (and writes into `out` where one is given)."""
    res = None
    for k, ((r0, n), wp) in enumerate(wslices):
        last = k == len(wslices) - 1
        res = dense_conv3x3(xp[:, r0:r0 + n], wp, None, beta if last else None, res, relu and last, out_f32 and last, out if last else None)
    return res


def dense_conv_applicable(imgs, H, W, Cin, Cout):
    """Shapes sdf_dense_conv3x3_fwd has an instantiation for (Cin <= 16 or Cin == 96, Cout in blocks of 32, 31-bit offsets)."""
    rec = -(-Cin // 16)
    return rec in (1, 6) and Cout % 32 == 0 and imgs * H * W * max(rec * 64, Cout * 4) < 1 << 31


def dense_conv3x3(xp, wplanes, alpha=None, beta=None, resid=None, relu=False, out_f32=False, out=None):
    """out = act(alpha * conv3x3(x, w) + beta (+ resid)), stride 1, zero padding 1 (sdf_dense_conv3x3_fwd).  xp / resid / the result
    are activation planes; out_f32 returns (imgs, H, W, N) fp32 (channels last) instead.  `out`: a preallocated contiguous tensor of the
    result's shape and dtype to write into (e.g. a slice of a larger buffer) instead of a fresh one."""
    imgs, rec, H, W, _ = xp.shape
    N = wplanes.shape[1]
    if wplanes.shape[2] != rec * 144:
        raise SdfError(f"weight planes of K = {wplanes.shape[2]} against {rec} activation records")
    # a channel slice xp = full[:, r0:r0 + rec] of a wider contiguous planes tensor is addressed in place
    if xp.stride()[1:] != (H * W * 32, W * 32, 32, 1) or xp.stride(0) % (H * W * 32) or xp.stride(0) < rec * H * W * 32:
        raise SdfError("activation planes must be contiguous or a record slice of a contiguous planes tensor")
    x_records = xp.stride(0) // (H * W * 32)
    if resid is not None and tuple(resid.shape) != (imgs, N // 16, H, W, 32):
        raise SdfError("residual planes must have the output's shape")
    shape, dtype = ((imgs, H, W, N), torch.float32) if out_f32 else ((imgs, N // 16, H, W, 32), torch.float16)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=xp.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device != xp.device:
        raise SdfError(f"out must be a contiguous {dtype} tensor of shape {shape} on the activations' device")
    d = DenseConvDesc()
    d.x, d.w, d.x_records = _ptr(xp, torch.float16), _ptr(wplanes, torch.float16), x_records
    d.alpha, d.beta = _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    d.resid, d.out = _ptr(resid, torch.float16), out.data_ptr()
    d.imgs, d.H, d.W, d.cin_records, d.N, d.relu, d.out_f32 = imgs, H, W, rec, N, int(relu), int(out_f32)
    d.acc_scale = _dense_scale(wplanes)
    _check(lib().sdf_dense_conv3x3_fwd(C.byref(d), _stream()), "sdf_dense_conv3x3_fwd")
    return out


# ---- Linear layer on real-valued activations (ANN swin blocks; csrc/dense_linear.hip) ----
def _dense_scale(wplanes):
    """1 / weight scale of dense fp16 planes made by pack_dense_linear_weight / pack_dense_conv_weight.  The scale travels as an attribute of
    the planes tensor: a copy (.to(), .clone(), a slice, a state_dict round trip) drops it, and the kernels would then return results
    wrong by a power of two - so a tensor without it is refused."""
    if not hasattr(wplanes, "sdf_acc_scale"):
        raise SdfError("dense fp16 weight planes without their scale: use the tensor returned by pack_dense_*_weight as is")
    return wplanes.sdf_acc_scale


def _f16_planes(w):
    """fp32 (N, K) -> fp16 planes (2, N, K) of s * w: hi = fp16(s w), lo = fp16(s w - hi), s the power of two that puts max|w| in
    [2^14, 2^15) - every weight within 2^-13 of the largest keeps 22 significant bits (unscaled, a weight of 0.02 has an fp16-subnormal
    lo half and keeps 19).  1 / s travels with the tensor as `sdf_acc_scale`; the kernels multiply the accumulator by it (exact)."""
    import math
    w = w.detach().float()
    mx = float(w.abs().max()) if w.numel() else 0.0
    scale = 2.0 ** (14 - math.floor(math.log2(mx))) if mx > 0 and math.isfinite(mx) else 1.0
    scale = min(max(scale, 2.0 ** -100), 2.0 ** 100)
    ws = w * scale
    hi = ws.half()
    planes = torch.stack([hi, (ws - hi.float()).half()]).contiguous()
    planes.sdf_acc_scale = 1.0 / scale
    return planes


def pack_dense_linear_weight(w):
    """Linear weight (N, K) fp32 -> scaled fp16 planes (2, N, K) (see _f16_planes)."""
    return _f16_planes(w)


def dense_linear_applicable(M, N, K):
    return N % 96 == 0 and K % 32 == 0 and M * max(N, K) * 4 < 1 << 31


def dense_linear(a, wplanes, bias=None, gelu=False, resid=None, out=None):
    """out = act(a @ w.T + bias) (+ resid) for a (M, K) fp32, w as fp16 planes (2, N, K) (sdf_dense_linear_fwd); `out` may be
    `resid` (in-place shortcut add)."""
    M, K = a.shape
    N = wplanes.shape[1]
    if wplanes.shape[2] != K or not a.is_contiguous():
        raise SdfError("dense_linear needs a contiguous (M, K) activation and (2, N, K) weight planes")
    if resid is not None and (tuple(resid.shape) != (M, N) or not resid.is_contiguous()):
        raise SdfError("residual must be a contiguous (M, N) tensor")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    d = DenseLinearDesc()
    d.a, d.w, d.bias, d.resid, d.out = _ptr(a, torch.float32), _ptr(wplanes, torch.float16), _ptr(bias, torch.float32), _ptr(resid, torch.float32), _ptr(out, torch.float32)
    d.M, d.N, d.K, d.gelu = M, N, K, int(gelu)
    d.acc_scale = _dense_scale(wplanes)
    _check(lib().sdf_dense_linear_fwd(C.byref(d), _stream()), "sdf_dense_linear_fwd")
    return out


def linear_train_applicable(M, N, K):
    return N % 96 == 0 and K % 96 == 0 and M * max(N, K) * 4 < 1 << 31


def linear_train(a, w, bias=None, mode=0, conv_wp=0):
    """Training-path Linear products from fp32 tensors (sdf_linear_train_fwd).  mode 0: a (M, K) spikes @ w.T + bias -> (M, N);
    mode 1: a = dY (M, N) @ w -> (M, K).  w is the layer's (N, K) fp32 weight as it is.  conv_wp > 0 (mode 0): the convolution form -
    a (M, C) ringed channels-last rows, w (N, 9 C) ordered (ky, kx, c), result on the ringed grid."""
    N, K = w.shape
    M = a.shape[0]
    if a.shape[1] != ((K // 9 if conv_wp else K) if mode == 0 else N) or not a.is_contiguous() or not w.is_contiguous():
        raise SdfError("linear_train needs contiguous a (M, K | N) and w (N, K)")
    out = torch.empty((M, N if mode == 0 else K), dtype=torch.float32, device=a.device)
    d = LinearTrainDesc()
    d.a, d.w, d.bias, d.out = _ptr(a, torch.float32), _ptr(w, torch.float32), _ptr(bias if mode == 0 else None, torch.float32), _ptr(out, torch.float32)
    d.M, d.N, d.K, d.mode = M, N, K, mode
    d.cv_C, d.cv_Wp = (K // 9, conv_wp) if conv_wp else (0, 0)
    _note(flop=2.0 * M * N * K, bytes=4.0 * M * (N + a.shape[1]), what=f"linear {'fwd' if mode == 0 else 'dX'} {M}x{N}x{K}")
    _check(lib().sdf_linear_train_fwd(C.byref(d), _stream()), "sdf_linear_train_fwd")
    return out


def linear_dw_applicable(M, N, K):
    return N % 96 == 0 and K % 96 == 0 and M * max(N, K) * 4 < 1 << 31


def linear_dw(dy, x, conv_wp=0):
    """dW (N, K) = dy.T @ x for dy (M, N) fp32 and x (M, K) fp32 holding spikes (values exact in bf16) - the weight gradient of a
    spike-fed Linear layer (sdf_linear_dw_fwd): dy split into three bf16 planes in the kernel, fp32 accumulation, m ranges summed in a
    fixed order.  conv_wp > 0: the convolution form on zero-ringed channels-last pixel rows (see conv3x3_dw) -> (N, 9 C)."""
    M, N = dy.shape
    Cx = x.shape[1]
    K = 9 * Cx if conv_wp else Cx
    if x.shape[0] != M or not dy.is_contiguous() or not x.is_contiguous():
        raise SdfError("linear_dw needs contiguous (M, N) and (M, K) operands")
    ns = lib().sdf_linear_dw_splits(M, N, K, Cx if conv_wp else 0)
    if ns < 1:
        raise SdfError(f"sdf_linear_dw_fwd: unsupported shape M={M} N={N} K={K} (N and K must be multiples of 96)")
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    part = torch.empty((ns, N, K), dtype=torch.float32, device=dy.device) if ns > 1 else None
    d = LinearDwDesc()
    d.dy, d.x, d.dw, d.partial = _ptr(dy, torch.float32), _ptr(x, torch.float32), _ptr(dw, torch.float32), _ptr(part, torch.float32)
    d.M, d.N, d.K, d.nsplit = M, N, K, ns
    d.cv_C, d.cv_Wp = (Cx, conv_wp) if conv_wp else (0, 0)
    _note(flop=2.0 * M * N * K, bytes=4.0 * M * (N + Cx), what=f"linear dW {M}x{N}x{K}")
    _check(lib().sdf_linear_dw_fwd(C.byref(d), _stream()), "sdf_linear_dw_fwd")
    return dw


def conv3x3_dw_applicable(imgs, Cin, Cout, H, W):
    return Cin % 96 == 0 and Cout % 96 == 0 and imgs * (H + 2) * (W + 2) * max(Cin, Cout) * 4 < 1 << 31


def ringed_rows(t):
    """(imgs, C, H, W) fp32 -> zero-ringed channels-last pixel rows (imgs * (H + 2) * (W + 2), C) (sdf_ringed_rows_fwd)."""
    imgs, Cc, H, W = t.shape
    if not t.is_contiguous():
        raise SdfError("ringed rows need a contiguous (imgs, C, H, W) tensor")
    out = torch.empty((imgs * (H + 2) * (W + 2), Cc), dtype=torch.float32, device=t.device)
    _check(lib().sdf_ringed_rows_fwd(_ptr(t, torch.float32), out.data_ptr(), imgs, Cc, H, W, _stream()), "sdf_ringed_rows_fwd")
    return out


def unring_rows(rows, imgs, Cc, H, W, bias=None):
    """Ringed channels-last rows (imgs * (H + 2) * (W + 2), C) -> (imgs, C, H, W) (+ bias) (sdf_unring_rows_fwd)."""
    if tuple(rows.shape) != (imgs * (H + 2) * (W + 2), Cc) or not rows.is_contiguous():
        raise SdfError("unring_rows: shape does not match the ringed grid")
    out = torch.empty((imgs, Cc, H, W), dtype=torch.float32, device=rows.device)
    _check(lib().sdf_unring_rows_fwd(_ptr(rows, torch.float32), _ptr(bias, torch.float32), out.data_ptr(),
                                     imgs, Cc, H, W, _stream()), "sdf_unring_rows_fwd")
    return out


def conv3x3_fwd_ringed(xr, weight, bias, imgs, H, W):
    """Forward of a 3x3 / stride 1 / pad 1 convolution on the ringed rows xr (imgs * (H + 2) * (W + 2), Cin) of a SPIKE image ->
    (imgs, Cout, H, W) fp32 (sdf_linear_train_fwd, convolution form + sdf_unring_rows_fwd)."""
    N = weight.shape[0]
    w9 = weight.detach().float().permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    return unring_rows(linear_train(xr, w9, None, mode=0, conv_wp=W + 2), imgs, N, H, W, bias)


_ringed_rows = ringed_rows


def conv3x3_dw(dy, x):
    """Weight gradient (Cout, Cin, 3, 3) of a 3x3 / stride 1 / pad 1 convolution fed by spikes: dy (imgs, Cout, H, W), x (imgs, Cin,
    H, W) fp32 NCHW as the training path holds them (sdf_linear_dw_fwd, convolution form).  Both go to zero-ringed channels-last
    pixel rows first - on that grid a tap is a row offset, and the zero ring of dy removes what a row offset wraps around an image
    edge."""
    imgs, N, H, W = dy.shape
    Cc = x.shape[1]
    if tuple(x.shape) != (imgs, Cc, H, W) and tuple(x.shape) != (imgs * (H + 2) * (W + 2), Cc):
        raise SdfError("conv3x3_dw needs dy (imgs, Cout, H, W) and x (imgs, Cin, H, W) or its ringed rows")
    xr = x if x.dim() == 2 else ringed_rows(x.contiguous())           # (the forward may have kept the ringed rows)
    dw = linear_dw(ringed_rows(dy), xr, conv_wp=W + 2)
    return dw.view(N, 3, 3, Cc).permute(0, 3, 1, 2).contiguous()


def layer_norm(x, gamma, beta, eps):
    """LayerNorm over the last dim of a contiguous fp32 tensor (sdf_layer_norm_fwd)."""
    Cc = x.shape[-1]
    if not x.is_contiguous():
        raise SdfError("layer_norm needs a contiguous tensor")
    out = torch.empty_like(x)
    _check(lib().sdf_layer_norm_fwd(_ptr(x, torch.float32), _ptr(gamma, torch.float32), _ptr(beta, torch.float32), out.data_ptr(),
                                    x.numel() // Cc, Cc, eps, _stream()), "sdf_layer_norm_fwd")
    return out


def dense_conv3x3_strided(x_cl, wplanes, bias, stride, out_T=0):
    """3x3 / pad 1 / stride `stride` convolution of a channels-last fp32 image x_cl (imgs, H, W, C) as a GEMM over gathered rows
    (sdf_dense_linear_fwd, convolution form) -> (imgs, OH, OW, N) fp32 channels last; with out_T = T the images, (t, b)-major on the
    way in, leave (b, t)-major.  wplanes = pack_dense_linear_weight(w.permute(0, 2, 3, 1).reshape(N, 9 * C))."""
    imgs, H, W, Cc = x_cl.shape
    N = wplanes.shape[1]
    if wplanes.shape[2] != 9 * Cc or not x_cl.is_contiguous():
        raise SdfError("dense_conv3x3_strided needs a contiguous (imgs, H, W, C) image and (2, N, 9C) weight planes")
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((imgs, OH, OW, N), dtype=torch.float32, device=x_cl.device)
    d = DenseLinearDesc()
    d.a, d.w, d.bias, d.resid, d.out = _ptr(x_cl, torch.float32), _ptr(wplanes, torch.float16), _ptr(bias, torch.float32), None, _ptr(out)
    d.M, d.N, d.K, d.gelu = imgs * OH * OW, N, 9 * Cc, 0
    d.cv_H, d.cv_W, d.cv_C, d.cv_stride, d.cv_OH, d.cv_OW, d.out_T = H, W, Cc, stride, OH, OW, out_T
    d.acc_scale = _dense_scale(wplanes)
    _check(lib().sdf_dense_linear_fwd(C.byref(d), _stream()), "sdf_dense_linear_fwd")
    return out


def pack_conv_weight(w, nsplit=3, cin_pad=None):
    """Conv2d weight (Cout, Cin, KH, KW) fp32 -> bf16 planes (nsplit, Cout, KH*KW*Cin_pad) in (ky, kx, cin) K order
    (zero rows for padded input channels)."""
    Cout, Cin, KH, KW = w.shape
    cp = Cin if cin_pad is None else cin_pad
    wk = torch.zeros((Cout, KH, KW, cp), dtype=torch.float32, device=w.device)
    wk[..., :Cin] = w.detach().float().permute(0, 2, 3, 1)
    return split_weight(wk.reshape(Cout, KH * KW * cp), nsplit)


def spike_conv2d(x, Wp, imgs, H, W, Cin, OH, OW, KH, KW, stride, dy, dx, out=None, out_spike=None, alpha=None, beta=None,
                 resid=None, out_rowmap=None, sn=None, sn_T=0, pos=None):
    """sdf_spike_conv2d_fwd.  x: u8 spikes NHWC (imgs,H,W,Cin); Wp: planes (nsplit, Cout, KH*KW*Cin).
    fp32 epilogue -> `out` (rows, Cout); fused neuron (sn, sn_T=10, pos=(count, inner, ostride, t_stride)) -> `out_spike`."""
    d = _conv_desc(x, Wp, imgs, H, W, Cin, OH, OW, KH, KW, stride, dy, dx, out, out_spike, alpha, beta, resid, out_rowmap, sn, sn_T, pos)
    g = d.g
    _note(flop=2 * g.M * g.N * g.K, shape=(int(g.M), int(g.N), int(g.K)), fused_neuron=sn is not None)
    _check(lib().sdf_spike_conv2d_fwd(C.byref(d), _stream()), "sdf_spike_conv2d_fwd")
    return out if sn is None else out_spike


def spike_conv2d_multi(x, classes, imgs, H, W, Cin, OH, OW, out, alpha=None, beta=None):
    """sdf_spike_conv2d_multi_fwd: up to four stride-1 convolutions of the same spike images into the same fp32 buffer that differ only in
    taps, weights and output row map - `classes` = [{"Wp", "KH", "KW", "dy", "dx", "rowmap"}, ...], the output-parity classes of a
    transposed convolution - as one launch where the library can (else one call each)."""
    arr = (SpikeConvDesc * len(classes))()
    flop = 0
    for i, c in enumerate(classes):
        d = _conv_desc(x, c["Wp"], imgs, H, W, Cin, OH, OW, c["KH"], c["KW"], 1, c["dy"], c["dx"], out, None, alpha, beta, None, c["rowmap"],
                       None, 0, None)
        C.memmove(C.byref(arr, i * C.sizeof(SpikeConvDesc)), C.byref(d), C.sizeof(SpikeConvDesc))
        flop += 2 * d.g.M * d.g.N * d.g.K
    _note(flop=flop, shape=(int(arr[0].g.M), int(arr[0].g.N), len(classes)))
    _check(lib().sdf_spike_conv2d_multi_fwd(arr, len(classes), _stream()), "sdf_spike_conv2d_multi_fwd")
    return out


def _conv_desc(x, Wp, imgs, H, W, Cin, OH, OW, KH, KW, stride, dy, dx, out, out_spike, alpha, beta, resid, out_rowmap, sn, sn_T, pos):
    d = SpikeConvDesc()
    g = d.g
    g.A, g.Wp = _ptr(x, torch.uint8), _ptr(Wp)
    g.M, g.N, g.K = imgs * OH * OW, Wp.shape[1], KH * KW * Cin
    g.lda, g.ldo, g.nsplit, g.acc_scale = 0, Wp.shape[1], Wp.shape[0], _acc_scale(Wp)
    if Wp.dtype == torch.int8:                                    # digit planes (split_weight_i8x3)
        g.nsplit, g.col_scale = (PLANES_I8X3_TILED if getattr(Wp, "sdf_tiled", False) else PLANES_I8X3), _ptr(Wp.sdf_col_scale, torch.float32)
    elif Wp.dtype != torch.int16:
        raise SdfError(f"weight planes must be int16 (16-bit float planes) or int8 (digit planes), got {Wp.dtype}")
    g.alpha, g.beta = _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    g.resid, g.out_rowmap = _ptr(resid, torch.float32), _ptr(out_rowmap, torch.int32)
    if out_rowmap is not None and out is not None:
        g.out_rows = out.numel() // g.ldo
    if sn is not None or Wp.dtype == torch.int8:
        _set_ws(g, x)                                             # (split-K scratch: the small-M digit convolution always splits)
    if sn is not None:
        g.out_spike = _ptr(out_spike, torch.uint8)
        g.out = _ptr(out, torch.float32)                          # optional membrane output (pre-activation + resid)
        g.sn_T, g.sn_kind, g.tau, g.v_th = sn_T, KIND[sn.kind], sn.tau, sn.v_th
        g.soft_reset, g.v_reset = _reset(sn.v_reset)
        g.psn_w, g.psn_b = _ptr(sn.psn_w, torch.float32), _ptr(sn.psn_b, torch.float32)
        g.pos_count, g.pos_inner, g.pos_ostride, g.t_stride = pos
    else:
        g.out = _ptr(out, torch.float32)
        _set_ws(g, x)
    d.H, d.W, d.Cin, d.OH, d.OW, d.KH, d.KW, d.sy, d.sx = H, W, Cin, OH, OW, KH, KW, stride, stride
    for i in range(3):
        d.dy[i] = dy[i] if i < len(dy) else 0
        d.dx[i] = dx[i] if i < len(dx) else 0
    return d


def head_conv_sn_supported(T, H, W, Cin, Cout):
    """Shapes sdf_head_conv_sn_fwd is built for (see include/sdformerflow_hip.h)."""
    return (Cin, Cout) in ((2, 32), (2, 48), (2, 64), (4, 48)) and T in (5, 10, 20) and W % 16 == 0


def head_conv_sn(x, w, B, T, H, W, p: NeuronParams, alpha=None, beta=None, voxel_bins=None):
    """sdf_head_conv_sn_fwd: x (B*T,H,W,Cin) fp32 NHWC, w (Cout,Cin,3,3) fp32 -> u8 spikes (B,T,H,W,Cout).
    With `voxel_bins`, x is the event voxel (B, bins, 2, H, W) itself, read in place through strides: input channel ci of time
    step t is polarity ci % 2 of bin (ci // 2) * T + t (reference patch embedding, Spiking_modules.py:1775-1784)."""
    Cout, Cin = w.shape[0], w.shape[1]
    if not x.is_contiguous() or not w.is_contiguous():
        raise SdfError("head_conv_sn needs a contiguous input and OIHW weights")
    out = torch.empty((B, T, H, W, Cout), dtype=torch.uint8, device=x.device)
    d = HeadConvDesc()
    if voxel_bins is not None:
        if tuple(x.shape) != (B, voxel_bins, 2, H, W) or Cin * T > 2 * voxel_bins or Cin > 4:
            raise SdfError(f"voxel {tuple(x.shape)} does not hold {Cin} channels x {T} steps")
        hw = H * W
        d.x_sb, d.x_st, d.x_sy, d.x_sx = voxel_bins * 2 * hw, 2 * hw, W, 1
        for ci in range(Cin):
            d.x_sc[ci] = (ci // 2) * T * 2 * hw + (ci % 2) * hw
    d.x, d.w, d.out = _ptr(x, torch.float32), _ptr(w, torch.float32), _ptr(out, torch.uint8)
    d.alpha, d.beta = _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    d.B, d.T, d.H, d.W, d.Cin, d.Cout = B, T, H, W, Cin, Cout
    d.sn_kind, d.tau, d.v_th = KIND[p.kind], p.tau, p.v_th
    d.soft_reset, d.v_reset = _reset(p.v_reset)
    d.psn_w, d.psn_b = _ptr(p.psn_w, torch.float32), _ptr(p.psn_b, torch.float32)
    _check(lib().sdf_head_conv_sn_fwd(C.byref(d), _stream()), "sdf_head_conv_sn_fwd")
    return out


def flow_out(pred, H, W, scale_y, scale_x):
    """sdf_flow_out_fwd: pred (B,D,h,w,C) fp32 (last-dim stride 1, rows ldp floats apart) -> (B,C,H,W) = nearest-upsampled time sum."""
    B, D, h, w, Cc = pred.shape
    if pred.stride(4) != 1 or pred.stride(2) != w * pred.stride(3) or pred.stride(1) != h * pred.stride(2) or pred.stride(0) != D * pred.stride(1):
        raise SdfError("flow_out needs a (B,D,h,w,C) view of a dense (rows, ldp) buffer")
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=pred.device)
    _check(lib().sdf_flow_out_fwd(_ptr(pred, torch.float32), out.data_ptr(), B, D, h, w, pred.stride(3), Cc, H, W, scale_y, scale_x,
                                  _stream()), "sdf_flow_out_fwd")
    return out


def pointwise_conv_supported(Cin, N):
    return Cin == 96 and N in (96, 192)


def pointwise_conv_f32(x, w, stride, bias=None):
    """sdf_pointwise_conv_f32_fwd: x (imgs,H,W,Cin) fp32 NHWC, w (N,Cin) fp32 -> (imgs,OH,OW,N) fp32, exact fp32 MFMA."""
    imgs, H, W, Cin = x.shape
    N = w.shape[0]
    if not x.is_contiguous() or not w.is_contiguous() or tuple(w.shape) != (N, Cin):
        raise SdfError("pointwise_conv_f32 needs a contiguous NHWC image and an (N, Cin) weight")
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((imgs, OH, OW, N), dtype=torch.float32, device=x.device)
    d = PointwiseConvDesc()
    d.x, d.w, d.bias, d.out = _ptr(x, torch.float32), _ptr(w, torch.float32), _ptr(bias, torch.float32), out.data_ptr()
    d.imgs, d.H, d.W, d.Cin, d.N, d.stride, d.OH, d.OW = imgs, H, W, Cin, N, stride, OH, OW
    _check(lib().sdf_pointwise_conv_f32_fwd(C.byref(d), _stream()), "sdf_pointwise_conv_f32_fwd")
    return out


def pred_head_supported(D, Cin, H, W, h, w, sn, sn_next=None):
    """Mirror of sdf_pred_head_fwd's shape rules (csrc/pred_head.hip): the caller keeps the three-launch form otherwise."""
    if Cin not in (96, 192, 384) or D not in (5, 10, 20) or H % h or W % w:
        return False
    if sn.kind not in KIND or (sn_next is not None and sn_next.kind not in KIND):       # (GLIF: the general launch only)
        return False
    if sn.kind == "psn" and D > 10:
        return False
    return sn_next is None or sn_next.kind == sn.kind or {sn.kind, sn_next.kind} <= {"lif", "if"}


def pred_head(z, wgt, bias, sn, H, W, want_pred=True, nxt=None, keep=False):
    """sdf_pred_head_fwd: z (B,D,h,w,Cin) fp32 channel-last -> (pred (B,D,h,w,4) fp32 or None, flow (B,2,H,W) fp32, spikes of
    SN_pred(z) (B,D,h,w,Cin) u8 if `keep`).  `nxt` = (spike image (B,D,h,w,ld) u8 of the next decoder level, its neuron,
    offset of z's slice, offset of the prediction's 4-wide slice, (offset, length) of the padding channels to zero)."""
    B, D, h, w, Cin = z.shape
    d = PredHeadDesc()
    d.z, d.B, d.D, d.h, d.w, d.Cin = _ptr(z, torch.float32), B, D, h, w, Cin
    _ncfg(d.sn_pred, sn)
    d.wgt, d.bias = _ptr(wgt, torch.float32), _ptr(bias, torch.float32)
    pred = torch.empty((B, D, h, w, 4), dtype=torch.float32, device=z.device) if want_pred else None
    flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=z.device) if H is not None else None
    d.pred, d.flow, d.H, d.W = _ptr(pred), _ptr(flow), H or 0, W or 0
    if nxt is not None:
        img, sn_next, z_off, p_off, (zero_off, zero_len) = nxt
        if img.dtype != torch.uint8 or not img.is_contiguous() or tuple(img.shape[:4]) != (B, D, h, w):
            raise SdfError("the next level's spike image must be a contiguous (B,D,h,w,ld) u8 tensor")
        d.next_spikes, d.next_ld, d.next_z_off, d.next_pred_off = img.data_ptr(), img.shape[4], z_off, p_off
        d.next_zero_off, d.next_zero_len = zero_off, zero_len
        _ncfg(d.sn_next, sn_next)
    sp = torch.empty((B, D, h, w, Cin), dtype=torch.uint8, device=z.device) if keep else None
    d.keep_spikes = _ptr(sp)
    _check(lib().sdf_pred_head_fwd(C.byref(d), _stream()), "sdf_pred_head_fwd")
    return pred, flow, sp


def deconv2x2_applicable(imgs, T, H, W, Cin, Cout, fast_only=False):
    """Mirror of sdf_spike_deconv3x3s2_fwd's shape rules (csrc/spike_gemm.hip).  `fast_only`: only where the halo-tile kernel
    (csrc/spike_deconv_wres.hip: 208 padded input channels, at least 4 096 input pixels) serves it - the row-loop kernel's form of the
    product, which takes every other admitted shape, is slower than the parity-class launches it would replace."""
    if sw("SDF_DECONV_GEMM", "1") == "0" or sw("SDF_RES", "1") == "0":
        return False
    rows = imgs * H * W
    ok = T in (10, 20) and imgs % T == 0 and Cin % 16 == 0 and 16 <= Cin <= 256 and Cout % 8 == 0 and Cout >= 8 and \
        rows * Cin < 1 << 31 and rows * 16 * Cout < 1 << 31
    if fast_only:
        ok = ok and Cin == 208 and rows >= 4096 and sw("SDF_DECONV_WRES", "1") != "0"
    return ok


def pack_deconv2x2_weight(w, cin_pad):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) weight (Cin, Cout, 3, 3) -> int8 digit planes of the (4 Cout, 4 cin_pad)
    matrix of sdf_spike_deconv3x3s2_fwd: row (2 py + px) Cout + co, column q cin_pad + c with q = dh + 2 dw the neighbour (a + dh, b + dw);
    output row 2a + py takes kernel row 1 from input row a when py = 0, kernel rows 2 / 0 from input rows a / a + 1 when py = 1 (columns alike)."""
    Cin, Cout = w.shape[:2]
    w = w.detach().float()
    M = torch.zeros((4 * Cout, 4 * cin_pad), dtype=torch.float32, device=w.device)
    tap = {(0, 0): 1, (1, 0): 2, (1, 1): 0}                      # (output parity, input offset) -> kernel index
    for py in range(2):
        for px in range(2):
            for dh in range(2):
                for dw in range(2):
                    if (py, dh) in tap and (px, dw) in tap:
                        q, cls = dh + 2 * dw, 2 * py + px
                        M[cls * Cout:(cls + 1) * Cout, q * cin_pad:q * cin_pad + Cin] = w[:, :, tap[(py, dh)], tap[(px, dw)]].t()
    return split_weight_i8x3(M)


def spike_deconv3x3s2(s, planes, imgs, T, H, W, Cin, Cout, alpha=None, beta=None, out=None, tiled_bn=False):
    """sdf_spike_deconv3x3s2_fwd: s (imgs, H, W, Cin) u8 -> (imgs, 2H, 2W, Cout) fp32 = BN(ConvTranspose2d(3, 2, 1, 1)(s)), one launch.
    alpha / beta: (Cout), or with `tiled_bn` already repeated to the product's (4 Cout) columns."""
    if out is None:
        out = torch.empty((imgs, 2 * H, 2 * W, Cout), dtype=torch.float32, device=s.device)
    d = SpikeDeconvDesc()
    d.spikes, d.digits, d.cscale = _ptr(s, torch.uint8), _ptr(planes, torch.int8), _ptr(planes.sdf_col_scale, torch.float32)
    if alpha is not None and not tiled_bn:
        alpha, beta = alpha.repeat(4).contiguous(), beta.repeat(4).contiguous()
    d.alpha, d.beta = _ptr(alpha, torch.float32), _ptr(beta, torch.float32)
    d.out, d.imgs, d.T, d.H, d.W, d.Cin, d.Cout = _ptr(out, torch.float32), imgs, T, H, W, Cin, Cout
    _check(lib().sdf_spike_deconv3x3s2_fwd(C.byref(d), _stream()), "sdf_spike_deconv3x3s2_fwd")
    return out


def deconv_col2im(Y, imgs, H, W, Cout, alpha=None, beta=None, out=None):
    """sdf_deconv_col2im_fwd: Y (imgs*H*W, 9*Cout) fp32 per-tap products -> (imgs, 2H, 2W, Cout) fp32, BN fused."""
    if out is None:
        out = torch.empty((imgs, 2 * H, 2 * W, Cout), dtype=torch.float32, device=Y.device)
    _check(lib().sdf_deconv_col2im_fwd(_ptr(Y, torch.float32), _ptr(alpha, torch.float32), _ptr(beta, torch.float32),
                                       _ptr(out, torch.float32), imgs, H, W, Cout, _stream()), "sdf_deconv_col2im_fwd")
    return out


EVENT_VOXEL_MODES = {"signed": 0, "split": 1, "polarities": 2}
_EV_WS, _EV_TB_WS = {}, {}


def _stream_ws(cache, dev, need):
    """One scratch buffer per (device, stream) and entry-point family: calls on different streams must not share partial results."""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    if key not in cache or cache[key].numel() < need:
        cache[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return cache[key]


def _event_lists(fn, x, y, t, p, offsets, xy_kinds):
    """What the three event front ends (event_voxel, event_voxel_tb, event_iwe) check alike: x, y, t, p are 1-D GPU arrays of one
    length, x and y of one dtype the entry point takes (`xy_kinds` words them; `fn` prefixes every message).  Returns the arrays
    contiguous, n, the list offsets as ints and as the descriptor's host array (keep it alive), and the descriptor's xy_dtype."""
    for a in (x, y, t, p):
        _ptr(a)                                                          # (CPU tensors are refused, as everywhere)
    n = int(t.numel())
    if not (x.numel() == y.numel() == p.numel() == n and x.dim() == y.dim() == t.dim() == p.dim() == 1):
        raise SdfError(f"{fn}: x, y, t, p are 1-D arrays of one length")
    if x.dtype != y.dtype:
        raise SdfError(f"{fn}: x and y differ in dtype")
    xy = {torch.float32: 0, torch.int32: 1, torch.uint16: 2}.get(x.dtype)
    if xy is None:
        raise SdfError(f"{fn}: x, y are {xy_kinds}, not {x.dtype}")
    offs = [0, n] if offsets is None else [int(o) for o in offsets]
    return x.contiguous(), y.contiguous(), t.contiguous(), p.contiguous(), n, offs, (C.c_int64 * len(offs))(*offs), xy


def _event_t_range(fn, t, offs, n):
    """The descriptor's host array t_range = {t_first, t_last} per list, read back in one small copy: the library refuses a non-empty
    list whose two times are equal (keep the array alive across the calls)."""
    B = len(offs) - 1
    ends = [i for b in range(B) if offs[b + 1] > offs[b] for i in (offs[b], offs[b + 1] - 1)]
    if any(i < 0 or i >= n for i in ends):
        raise SdfError(f"{fn}: offsets outside the event arrays")
    got = iter(t[torch.tensor(ends, device=t.device, dtype=torch.long)].tolist())
    flat = [v for b in range(B) for v in ((next(got), next(got)) if offs[b + 1] > offs[b] else (0.0, 1.0))]
    return (C.c_float * (2 * B))(*flat)


def _event_rectify_map(fn, d, rectify_map):
    """`rectify_map` (H_s, W_s, 2) fp32 into the descriptor; returns the contiguous tensor (keep it alive across the calls)."""
    if rectify_map.dim() != 3 or rectify_map.shape[2] != 2:
        raise SdfError(f"{fn}: rectify_map is (H_s, W_s, 2)")
    rectify_map = rectify_map.contiguous()
    d.rectify_map, d.map_h, d.map_w = _ptr(rectify_map, torch.float32), rectify_map.shape[0], rectify_map.shape[1]
    return rectify_map


def _event_gather(fn, d, cache, need, refused, shape, out, n, dev):
    """The tail the three event front ends share, on a descriptor filled up to the geometry: workspace of `need` bytes (<= 0: the
    library refused the geometry - `refused` says which), `out` (None: a new tensor of `shape`), keys | stable sort | gather.
    `fn` names the entry-point pair sdf_<fn>_keys_fwd / sdf_<fn>_gather_fwd and prefixes the messages."""
    if need <= 0:
        raise SdfError(f"{fn}: geometry refused ({refused})", rc=E_SHAPE)
    ws = _stream_ws(cache, dev, need)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise SdfError(f"{fn}: out must be a contiguous {shape} tensor")
    d.out = _ptr(out, torch.float32)
    keys = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    d.keys = keys.data_ptr()
    _check(getattr(lib(), f"sdf_{fn}_keys_fwd")(C.byref(d), _stream()), f"sdf_{fn}_keys_fwd")
    if n:
        keys_sorted, order = torch.sort(keys, stable=True)               # plumbing: any stable sort serves
        d.keys_sorted, d.order = keys_sorted.data_ptr(), order.data_ptr()
    _check(getattr(lib(), f"sdf_{fn}_gather_fwd")(C.byref(d), _stream()), f"sdf_{fn}_gather_fwd")
    return out


def event_voxel(x, y, t, p, bins, sensor_size, offsets=None, crop=None, mode="signed", norm=None, spike_th=None, rectify_map=None,
                check=True, out=None):
    """Raw event lists -> voxel grid on the GPU (sdf_event_voxel_keys_fwd | stable sort | sdf_event_voxel_gather_fwd), with the semantics
    and the per-cell summation order of the reference's VoxelGrid on the CPU (DSEC_dataloader/event_representations.py:241-313): the
    result is bit-identical from run to run and independent of how lists are batched.

    x, y: fp32 (rectified, possibly fractional) - or int32 / uint16 sensor coordinates with `rectify_map` (H_s, W_s, 2) fp32, looked up
    as x, y <- map[y, x].  t, p: fp32, each list in time order.  `offsets`: B + 1 host ints cutting the arrays into B lists (None: one
    list).  `sensor_size` (H, W); `crop` (h, w): only the centre window is computed.
    mode "signed": (B, bins, h, w) | "split": the model's input (B, bins, 2, h, w) = relu(v) | relu(-v), with norm "minmax" / spike_th as
    harness.prepare_chunk applies them | "polarities": convert_CHW_polarities (B, bins, 2, h, w).
    A non-empty list whose first and last time are equal raises SdfError (`check` reads the two times back: one small copy; False
    skips it, and such a list then adds nothing)."""
    x, y, t, p, n, offs, host_offs, xy = _event_lists("event_voxel", x, y, t, p, offsets, "fp32, or int32 / uint16 with a rectify_map")
    if mode not in EVENT_VOXEL_MODES or norm not in (None, "minmax"):
        raise SdfError(f"event_voxel: unknown mode {mode!r} / norm {norm!r} (norm 'std' is harness.prepare_chunk's, on the un-normalised output)")
    B, (H, W) = len(offs) - 1, sensor_size
    h, w = crop if crop else (H, W)
    dev = t.device
    d = EventVoxelDesc()
    d.x, d.y, d.t, d.p, d.xy_dtype = x.data_ptr(), y.data_ptr(), _ptr(t, torch.float32), _ptr(p, torch.float32), xy
    if rectify_map is not None:
        rectify_map = _event_rectify_map("event_voxel", d, rectify_map)
    d.offsets, d.n_events = C.addressof(host_offs), n
    d.B, d.C, d.H, d.W, d.crop_h, d.crop_w = B, bins, H, W, (h if crop else 0), (w if crop else 0)
    d.mode, d.norm = EVENT_VOXEL_MODES[mode], int(norm == "minmax")
    d.use_spike_th, d.spike_th = int(spike_th is not None), float(spike_th or 0.0)
    if check and n:
        host_range = _event_t_range("event_voxel", t, offs, n)
        d.t_range = C.addressof(host_range)
    need = lib().sdf_event_voxel_workspace_bytes(n, B, bins, H, W, d.crop_h, d.crop_w)
    shape = (B, bins, h, w) if mode == "signed" else (B, bins, 2, h, w)
    return _event_gather("event_voxel", d, _EV_WS, need, f"B {B}, bins {bins}, sensor {H} x {W}, crop {crop}, {n} events", shape, out, n, dev)


def event_voxel_tb(x, y, t, p, num_bins, sensor_size, offsets=None, t_scale=1.0, crop=None, crop_origin=None, normalize=True,
                   mode="signed", lists_per_sample=1, norm=None, spike_th=None, want_event_mask=False, out=None):
    """Raw event lists -> the time-bilinear voxel grid of the MVSEC / MDR loaders on the GPU (sdf_event_voxel_tb_keys_fwd | stable sort |
    sdf_event_voxel_tb_gather_fwd), with the semantics and the per-cell summation order of the reference's
    EventSequenceToVoxelGrid_Pytorch on the CPU (MDR_dataloader/loader_utils.py:421-577): bit-identical from run to run and independent
    of how lists are batched.

    x, y: fp32, int32 or uint16 pixels (truncated to integers).  t: float64, each list in time order; `t_scale` multiplies it in
    float64 first (1e6 for the loaders' seconds).  p: fp32, 0 / 1 or -1 / +1.  `offsets`: L + 1 host ints cutting the arrays into L
    lists (None: one list).  `sensor_size` (H, W); `crop` (h, w) at `crop_origin` (oy, ox), default torchvision CenterCrop's
    int(round((H - h) / 2.0)).  `normalize`: each list by the mean / std of the non-zeros of its whole grid.
    mode "signed": (L, num_bins, h, w) | "polarities": the pol=False form (L, num_bins, 2, h, w) | "split": the model's input
    (L / lists_per_sample, lists_per_sample * num_bins, 2, h, w) = relu(v) | relu(-v) with a sample's lists (old, new) along the bins,
    norm "minmax" / spike_th as harness.prepare_chunk applies them; with `want_event_mask` returns (input, mask (B, 1, h, w) fp32)."""
    x, y, t, p, n, offs, host_offs, xy = _event_lists("event_voxel_tb", x, y, t, p, offsets, "fp32, int32 or uint16")
    if mode not in EVENT_VOXEL_MODES or norm not in (None, "minmax"):
        raise SdfError(f"event_voxel_tb: unknown mode {mode!r} / norm {norm!r} (norm 'std' is harness.prepare_chunk's, on the un-normalised output)")
    if mode != "split" and (norm or spike_th is not None or want_event_mask or lists_per_sample != 1):
        raise SdfError("event_voxel_tb: norm, spike_th, the event mask and paired lists belong to mode 'split'")
    L, (H, W) = len(offs) - 1, sensor_size
    if lists_per_sample not in (1, 2) or L < 1 or L % lists_per_sample:
        raise SdfError(f"event_voxel_tb: {L} lists do not make samples of {lists_per_sample}")
    h, w = crop if crop else (H, W)
    oy, ox = crop_origin if crop_origin is not None else ((int(round((H - h) / 2.0)), int(round((W - w) / 2.0))) if crop else (0, 0))
    dev = t.device
    d = EventVoxelTbDesc()
    d.x, d.y, d.t, d.p, d.xy_dtype = x.data_ptr(), y.data_ptr(), _ptr(t, torch.float64), _ptr(p, torch.float32), xy
    host_scale = C.c_double(float(t_scale))
    d.t_scale, d.offsets, d.n_events = C.addressof(host_scale), C.addressof(host_offs), n
    d.n_lists, d.lists_per_sample, d.nb, d.H, d.W = L, lists_per_sample, num_bins, H, W
    d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = (h if crop else 0), (w if crop else 0), oy, ox
    d.normalize, d.mode, d.norm = int(bool(normalize)), EVENT_VOXEL_MODES[mode], int(norm == "minmax")
    d.use_spike_th, d.spike_th = int(spike_th is not None), float(spike_th or 0.0)
    need = lib().sdf_event_voxel_tb_workspace_bytes(n, L, num_bins, H, W, d.crop_h, d.crop_w, oy, ox, d.normalize)
    shape = {"signed": (L, num_bins, h, w), "polarities": (L, num_bins, 2, h, w),
             "split": (L // lists_per_sample, lists_per_sample * num_bins, 2, h, w)}[mode]
    mask = torch.empty((shape[0], 1, h, w), dtype=torch.float32, device=dev) if want_event_mask else None
    d.event_mask = _ptr(mask, torch.float32)
    out = _event_gather("event_voxel_tb", d, _EV_TB_WS, need,
                        f"{L} lists, bins {num_bins}, sensor {H} x {W}, crop {crop} at {(oy, ox)}, {n} events", shape, out, n, dev)
    return (out, mask) if want_event_mask else out


EVENT_IWE_MODES = {"bilinear": 0, "nearest": 1}
IWE_STATS_FIELDS = ("sum", "sum_sq", "max", "n_nonzero")
_IWE_WS, _IWE_STATS_WS = {}, {}


def event_iwe(x, y, t, p, flow, sensor_size, offsets=None, crop=None, crop_origin=None, scale=1.0, t_ref=1.0, window=(0.0, 1.0),
              mode="bilinear", rectify_map=None, check=True, out=None):
    """Raw event lists + a flow -> the image of warped events on the GPU (sdf_event_iwe_keys_fwd | stable sort | sdf_event_iwe_gather_fwd;
    the definition: csrc/event_iwe.hip): (B, 2, h, w) fp32, channel 0 the p > 0 events and channel 1 the others,
    every event moved from its normalised time tau to `t_ref` along `scale` * the flow at its pixel.  Bit-identical from run to run and
    independent of how lists are batched; no float atomics.

    x, y, t, p, `offsets`, `rectify_map`, `check`: as hip.event_voxel takes them (t fp32, each list in time order).  flow (B, 2, h, w)
    fp32, channel 0 = x, on the output window: `crop` (h, w) of `sensor_size` (H, W) at `crop_origin` (oy, ox), default
    harness.center_crop's; no crop: the whole sensor.  `window` (a, b): only the events with a <= tn <= b, their time renormalised to
    the window.  mode "bilinear": four weighted corners, summed per cell in a fixed order | "nearest": 1 at the rounded position - the
    image holds integers.  The flow is looked up at the event's nearest pixel (a bilinear lookup is not built), and there is no
    backward pass: contrast-maximisation training is not served."""
    x, y, t, p, n, offs, host_offs, xy = _event_lists("event_iwe", x, y, t, p, offsets, "fp32, or int32 / uint16 with a rectify_map")
    if mode not in EVENT_IWE_MODES:
        raise SdfError(f"event_iwe: unknown mode {mode!r} (bilinear | nearest; a bilinear flow lookup, the average-timestamp image and "
                       "a backward pass are not built)")
    B, (H, W) = len(offs) - 1, sensor_size
    h, w = crop if crop else (H, W)
    oy, ox = crop_origin if crop_origin is not None else (((H - h) // 2, (W - w) // 2) if crop else (0, 0))
    if not crop and (oy, ox) != (0, 0):
        raise SdfError("event_iwe: crop_origin without a crop")
    a, b = (float(v) for v in window)
    if not (a < b) or not all(math.isfinite(v) for v in (a, b, float(t_ref))) or float(scale) != float(scale):
        raise SdfError(f"event_iwe: window {window!r} needs a < b, and finite window / t_ref / scale values", rc=E_SHAPE)
    _ptr(flow, torch.float32)
    if tuple(flow.shape) != (B, 2, h, w):
        raise SdfError(f"event_iwe: flow is {(B, 2, h, w)} on the output window, got {tuple(flow.shape)}")
    flow = flow.contiguous()
    dev = t.device
    d = EventIweDesc()
    d.x, d.y, d.t, d.p, d.xy_dtype = x.data_ptr(), y.data_ptr(), _ptr(t, torch.float32), _ptr(p, torch.float32), xy
    d.flow = flow.data_ptr()
    if rectify_map is not None:
        rectify_map = _event_rectify_map("event_iwe", d, rectify_map)
    d.offsets, d.n_events = C.addressof(host_offs), n
    d.B, d.H, d.W = B, H, W
    d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = (h if crop else 0), (w if crop else 0), oy, ox
    d.mode, d.scale, d.t_ref, d.win_a, d.win_b = EVENT_IWE_MODES[mode], float(scale), float(t_ref), a, b
    if check and n:
        host_range = _event_t_range("event_iwe", t, offs, n)
        d.t_range = C.addressof(host_range)
    need = lib().sdf_event_iwe_workspace_bytes(n, B, H, W, d.crop_h, d.crop_w, oy, ox, d.mode)
    return _event_gather("event_iwe", d, _IWE_WS, need, f"B {B}, sensor {H} x {W}, crop {crop} at {(oy, ox)}, {n} events", (B, 2, h, w),
                         out, n, dev)


def _record_table(fn, table, row, n, fields, dev):
    """The caller's table of per-sample fp64 records for a call that writes rows `row` .. `row` + n - 1: (rows, len(fields)) float64,
    contiguous, the rows inside it; None: a new zero table of row + n rows on `dev`.  Returns the table."""
    if table is None:
        table = torch.zeros((row + n, len(fields)), dtype=torch.float64, device=dev)
    _ptr(table, torch.float64)
    if table.dim() != 2 or table.shape[1] != len(fields) or not table.is_contiguous():
        raise SdfError(f"{fn}: table must be a contiguous (rows, {len(fields)}) float64 tensor")
    if row < 0 or row + n > table.shape[0]:
        raise SdfError(f"{fn}: rows {row} .. {row + n - 1} lie outside the table's {table.shape[0]}", rc=E_SHAPE)
    return table


def iwe_stats(iwe, table=None, row=0):
    """Per-sample statistics of an image of warped events on the GPU (sdf_iwe_stats_fwd: two launches, no read-back): sample b of iwe
    (B, 2, h, w) fp32 writes row `row` + b of `table` (rows, 4) float64 - IWE_STATS_FIELDS: sum, sum of squares, maximum and number of
    non-zero pixels of the channel sum - and leaves the other rows as they are.  `table` None: a new zero table of row + B rows.
    Returns the table.  fp64 sums in a fixed order: bit-identical from run to run and independent of B; exact on nearest images."""
    _ptr(iwe, torch.float32)
    if iwe.dim() != 4 or iwe.shape[1] != 2:
        raise SdfError(f"iwe_stats: iwe is (B, 2, h, w), got {tuple(iwe.shape)}")
    iwe = iwe.contiguous()
    B, _, H, W = iwe.shape
    dev = iwe.device
    table = _record_table("iwe_stats", table, row, B, IWE_STATS_FIELDS, dev)
    need = lib().sdf_iwe_stats_workspace_bytes(B, H, W)
    if need <= 0:
        raise SdfError(f"iwe_stats: geometry refused (B {B}, {H} x {W})", rc=E_SHAPE)
    ws = _stream_ws(_IWE_STATS_WS, dev, need)
    d = IweStatsDesc()
    d.iwe, d.table, d.workspace, d.workspace_bytes = iwe.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel()
    d.B, d.H, d.W, d.row0, d.rows = B, H, W, row, table.shape[0]
    _note(bytes=B * H * W * 8, shape=(B, H, W))
    _check(lib().sdf_iwe_stats_fwd(C.byref(d), _stream()), "sdf_iwe_stats_fwd")
    return table


FLOW_METRICS_FIELDS = ("n_valid", "sum_err", "n_pe1", "n_pe2", "n_pe3", "n_outlier", "sum_ang", "n_pixels")
_FM_WS, _PC_WS = {}, {}


def flow_metrics(pred, label, valid, event_mask=None, flow_scaling=1.0, table=None, row=0):
    """Per-sample sums of the evaluation metrics on the GPU (sdf_flow_metrics_fwd: two launches, no read-back): sample b of pred /
    label (B, 2, H, W), valid and event_mask (B, H, W) or (B, 1, H, W), all fp32, writes row `row` + b of `table` (rows, 8) float64 -
    FLOW_METRICS_FIELDS - and leaves the other rows as they are.  `table` None: a new zero table of row + B rows.  Returns the table.
    Per pixel the reference classes' fp32 arithmetic (loss.flow_supervised.AEE / AAE on one sample); fp64 sums in a fixed order:
    bit-identical from run to run and independent of B."""
    for a in (pred, label, valid):
        _ptr(a, torch.float32)
    if pred.dim() != 4 or pred.shape[1] != 2 or label.shape != pred.shape:
        raise SdfError(f"flow_metrics: pred and label are (B, 2, H, W), got {tuple(pred.shape)} and {tuple(label.shape)}")
    B, _, H, W = pred.shape

    def plane(t, name):
        if t.numel() != B * H * W or tuple(t.shape[-2:]) != (H, W):
            raise SdfError(f"flow_metrics: {name} is (B, H, W) or (B, 1, H, W) at the flow's size, got {tuple(t.shape)}")
        return t.contiguous()
    pred, label, valid = pred.contiguous(), label.contiguous(), plane(valid, "valid")
    if event_mask is not None:
        event_mask = plane(event_mask, "event_mask")
    dev = pred.device
    table = _record_table("flow_metrics", table, row, B, FLOW_METRICS_FIELDS, dev)
    need = lib().sdf_flow_metrics_workspace_bytes(B, H, W)
    if need <= 0:
        raise SdfError(f"flow_metrics: geometry refused (B {B}, {H} x {W})", rc=E_SHAPE)
    ws = _stream_ws(_FM_WS, dev, need)
    d = FlowMetricsDesc()
    d.pred, d.label, d.valid, d.event_mask = pred.data_ptr(), label.data_ptr(), valid.data_ptr(), _ptr(event_mask, torch.float32)
    d.table, d.workspace, d.workspace_bytes = table.data_ptr(), ws.data_ptr(), ws.numel()
    d.B, d.H, d.W, d.row0, d.rows, d.flow_scaling = B, H, W, row, table.shape[0], float(flow_scaling)
    _note(bytes=B * H * W * (5 + (event_mask is not None)) * 4, shape=(B, H, W))
    _check(lib().sdf_flow_metrics_fwd(C.byref(d), _stream()), "sdf_flow_metrics_fwd")
    return table


FLOW_LOSS_DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}          # SDF_FLOW_LOSS_F32 / _BF16 / _F16
FLOW_LOSS_FACTORS = (1, 2, 4, 8, 16)
_FL_WS = {}


def flow_loss(preds, label, mask, n_valid, flow_scaling=1.0, lambda_mod=1.0, grads=True, records=None, loss=None):
    """The supervised multi-scale flow loss and its gradient on the GPU (sdf_flow_loss_fwd: two launches whatever the number of levels,
    no read-back): `preds` a list of up to 8 raw decoder predictions (T_i, B, 2, h_i, w_i), contiguous, all fp32, bf16 or fp16, each a
    factor 1, 2, 4, 8 or 16 below label (B, 2, H, W) fp32; mask (B, H, W) or (B, 1, H, W) fp32; `n_valid` one fp32 on the device
    (train.global_valid_count).  What train.flow_loss_supervised computes on forward_train's summed, nearest-upsampled flows - per pixel
    the same fp32 operations, fp64 sums in a fixed order - without a full-resolution tensor per level.  Returns (loss, grads): loss a
    0-dim fp32 tensor; grads [d loss / d preds[i].sum(0)] as fp32 (B, 2, h_i, w_i) tensors, or None with `grads` False (loss only).
    `grads` a list of contiguous fp32 tensors: written into.  `records`: a contiguous (levels, B) float64 tensor receiving each level's
    per-sample sum of err * mask.  `loss`: a 1-element fp32 tensor to write into."""
    preds = list(preds)
    if not 1 <= len(preds) <= FLOW_LOSS_MAX_LEVELS:
        raise SdfError(f"flow_loss: 1 .. {FLOW_LOSS_MAX_LEVELS} prediction levels, got {len(preds)}", rc=E_SHAPE)
    for a in (label, mask, n_valid):
        _ptr(a, torch.float32)
    if label.dim() != 4 or label.shape[1] != 2:
        raise SdfError(f"flow_loss: label is (B, 2, H, W), got {tuple(label.shape)}")
    B, _, H, W = label.shape
    if mask.numel() != B * H * W or tuple(mask.shape[-2:]) != (H, W):
        raise SdfError(f"flow_loss: mask is (B, H, W) or (B, 1, H, W) at the label's size, got {tuple(mask.shape)}")
    if n_valid.numel() != 1:
        raise SdfError(f"flow_loss: n_valid is one fp32 value on the device, got {tuple(n_valid.shape)}")
    dtype = preds[0].dtype
    if dtype not in FLOW_LOSS_DTYPES:
        raise SdfError(f"flow_loss: predictions are float32, bfloat16 or float16, got {dtype}", rc=E_DTYPE)
    dev = label.device
    label, mask = label.contiguous(), mask.contiguous()
    want = grads is not False and grads is not None
    given = list(grads) if want and grads is not True else None
    if given is not None and len(given) != len(preds):
        raise SdfError(f"flow_loss: {len(given)} gradient tensors for {len(preds)} levels")
    d = FlowLossDesc()
    keep, out = [], []
    for i, p in enumerate(preds):
        _ptr(p, dtype)
        if p.dim() != 5 or p.shape[1] != B or p.shape[2] != 2:
            raise SdfError(f"flow_loss: level {i} is (T, {B}, 2, h, w), got {tuple(p.shape)}")
        T, h, w = p.shape[0], p.shape[3], p.shape[4]
        if h < 1 or w < 1 or H % h or W % w or H // h != W // w or H // h not in FLOW_LOSS_FACTORS:
            raise SdfError(f"flow_loss: level {i} at {h} x {w} is not a factor {FLOW_LOSS_FACTORS} below {H} x {W}", rc=E_SHAPE)
        if not 1 <= T <= 64:
            raise SdfError(f"flow_loss: level {i} has {T} time steps (1 .. 64)", rc=E_SHAPE)
        p = p.contiguous()
        keep.append(p)
        d.pred[i], d.h[i], d.w[i], d.T[i] = p.data_ptr(), h, w, T
        if want:
            g = torch.empty((B, 2, h, w), dtype=torch.float32, device=dev) if given is None else given[i]
            if _ptr(g, torch.float32) is None or tuple(g.shape) != (B, 2, h, w) or not g.is_contiguous():
                raise SdfError(f"flow_loss: the gradient of level {i} is a contiguous {(B, 2, h, w)} float32 tensor")
            out.append(g)
            d.grad[i] = g.data_ptr()
    if records is not None and (_ptr(records, torch.float64) is None or tuple(records.shape) != (len(preds), B)
                                or not records.is_contiguous()):
        raise SdfError(f"flow_loss: records is a contiguous {(len(preds), B)} float64 tensor")
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
    elif _ptr(loss, torch.float32) is None or loss.numel() != 1:
        raise SdfError("flow_loss: loss is a 1-element float32 tensor")
    need = lib().sdf_flow_loss_workspace_bytes(B, H, W, len(preds))
    if need <= 0:
        raise SdfError(f"flow_loss: geometry refused (B {B}, {H} x {W}, {len(preds)} levels)", rc=E_SHAPE)
    ws = _stream_ws(_FL_WS, dev, need)
    d.label, d.mask, d.n_valid, d.loss, d.records = label.data_ptr(), mask.data_ptr(), n_valid.data_ptr(), loss.data_ptr(), _ptr(records)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    d.levels, d.B, d.H, d.W, d.dtype = len(preds), B, H, W, FLOW_LOSS_DTYPES[dtype]
    d.flow_scaling, d.lambda_mod = float(flow_scaling), float(lambda_mod)
    _note(bytes=B * H * W * 12 + sum(p.numel() * p.element_size() for p in keep) + sum(g.numel() * 4 for g in out), shape=(B, H, W))
    _check(lib().sdf_flow_loss_fwd(C.byref(d), _stream()), "sdf_flow_loss_fwd")
    return loss.reshape(()), (out if want else None)


def prepare_chunk(voxel, crop=None, norm_input="minmax", spike_th=None, per_sample=False, out=None, crop_origin=None, event_mask=None):
    """harness.prepare_chunk(center_crop(voxel, crop), norm_input, spike_th, polarity=True) on the GPU without a host round trip
    (sdf_prepare_chunk_fwd), bit for bit: signed voxel (B, bins, Hs, Ws) fp32 -> the model's input (B, bins, 2, h, w).  `crop` (h, w) at
    `crop_origin` (default harness.center_crop's ((Hs - h) // 2, (Ws - w) // 2)).  norm_input "minmax" or None; "std" raises SdfError
    with rc E_DTYPE (harness.prepare_chunk serves it).  `per_sample`: min-max over each sample (what B batch-1 calls compute) instead
    of over the whole batch tensor (the reference's semantics).  `out`: a contiguous (B, bins, 2, h, w) tensor to write into.
    `event_mask`: a contiguous (B, 1, h, w) fp32 tensor that receives the loop's event mask, input.sum(1).sum(1, keepdim=True).bool()."""
    _ptr(voxel, torch.float32)
    if voxel.dim() != 4:
        raise SdfError(f"prepare_chunk: voxel is (B, bins, H, W), got {tuple(voxel.shape)}")
    voxel = voxel.contiguous()
    B, bins, Hs, Ws = voxel.shape
    h, w = crop if crop else (Hs, Ws)
    oy, ox = crop_origin if crop_origin is not None else (((Hs - h) // 2, (Ws - w) // 2) if crop else (0, 0))
    norm = {None: 0, "minmax": 1}.get(norm_input, 2)                    # (anything else is the library's to refuse)
    dev = voxel.device
    shape = (B, bins, 2, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise SdfError(f"prepare_chunk: out must be a contiguous {shape} tensor")
    if event_mask is not None and (tuple(event_mask.shape) != (B, 1, h, w) or not event_mask.is_contiguous()):
        raise SdfError(f"prepare_chunk: event_mask must be a contiguous {(B, 1, h, w)} tensor")
    need = lib().sdf_prepare_chunk_workspace_bytes(B)
    if need <= 0:
        raise SdfError(f"prepare_chunk: batch of {B} refused", rc=E_SHAPE)
    ws = _stream_ws(_PC_WS, dev, max(need, 256))
    d = PrepareChunkDesc()
    d.voxel, d.out, d.event_mask = voxel.data_ptr(), _ptr(out, torch.float32), _ptr(event_mask, torch.float32)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    d.B, d.bins, d.Hs, d.Ws = B, bins, Hs, Ws
    d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = (h if crop else 0), (w if crop else 0), oy, ox
    d.norm, d.per_sample = norm, int(bool(per_sample))
    d.use_spike_th, d.spike_th = int(spike_th is not None), float(spike_th or 0.0)
    _note(bytes=B * bins * h * w * 4 * (1 + 2 + 4 * (norm == 1 or spike_th is not None)), shape=shape)
    _check(lib().sdf_prepare_chunk_fwd(C.byref(d), _stream()), "sdf_prepare_chunk_fwd")
    return out


def _per_sample(fn, name, value, B, width):
    """`value` - one entry for every sample or a sequence of B - as a list of B entries (`width` > 1: each a tuple of that many)."""
    one = not isinstance(value, (list, tuple)) or (width > 1 and len(value) == width and not isinstance(value[0], (list, tuple)))
    rows = [value] * B if one else list(value)
    if len(rows) != B or (width > 1 and any(not isinstance(r, (list, tuple)) or len(r) != width for r in rows)):
        raise SdfError(f"{fn}: {name} is one entry or {B} of them (one per sample), got {value!r}")
    return rows


def augment_chunk(voxel, label, valid, crop, origins, flips, drop_q=None, drop_u=None, seed=0, offset=0, norm_input="minmax",
                  spike_th=None, per_sample=False, mask_events=False, out=None, label_out=None, mask_out=None, event_mask=None):
    """A loader item -> the training step's (input, label, mask) on the GPU without a host round trip (sdf_augment_chunk_fwd): the
    reference loops' crop, flips and event drop (DSEC_dataloader.data_augmentation), then harness.prepare_chunk and, with `mask_events`,
    mask * event_mask - bit for bit what that composition gives.  voxel (B, bins, Hs, Ws) fp32 signed; label (B, 2, Hs, Ws) fp32 and valid
    (B, 1, Hs, Ws) or (B, Hs, Ws), fp32 / uint8 / bool - either may be None, and so is its output.  `crop` (h, w) or None (the whole
    volume); `origins` one (oy, ox) or B of them; `flips` one flag word or B (bit 0 horizontal, bit 1 vertical); `drop_q` None, one
    value or B (None / negative: that sample keeps its events).  A dropped sample takes its uniform field from `drop_u` (B, bins, h, w)
    fp32 in output coordinates when given, else from the kernel's Philox4x32-10 keyed by `seed` at `offset` (64-bit each; the same pair
    gives the same field, a caller advances `offset` per step).  norm_input / spike_th / per_sample / event_mask as hip.prepare_chunk.
    Returns (out (B, bins, 2, h, w), label_out (B, 2, h, w) or None, mask_out (B, 1, h, w) fp32 or None); `out`, `label_out`,
    `mask_out`: contiguous tensors of those shapes to write into."""
    _ptr(voxel, torch.float32)
    if voxel.dim() != 4:
        raise SdfError(f"augment_chunk: voxel is (B, bins, H, W), got {tuple(voxel.shape)}")
    voxel = voxel.contiguous()
    B, bins, Hs, Ws = voxel.shape
    if B > AUGMENT_MAX_B:
        raise SdfError(f"augment_chunk: batch of {B} refused (at most {AUGMENT_MAX_B} per call)", rc=E_SHAPE)
    h, w = crop if crop else (Hs, Ws)
    dev = voxel.device
    if label is not None:
        _ptr(label, torch.float32)
        if tuple(label.shape) != (B, 2, Hs, Ws):
            raise SdfError(f"augment_chunk: label is {(B, 2, Hs, Ws)}, got {tuple(label.shape)}")
        label = label.contiguous()
    if valid is not None:
        _ptr(valid)
        if valid.numel() != B * Hs * Ws or tuple(valid.shape[-2:]) != (Hs, Ws):
            raise SdfError(f"augment_chunk: valid is (B, H, W) or (B, 1, H, W) at the voxel's size, got {tuple(valid.shape)}")
        if valid.dtype == torch.bool:
            valid = valid.contiguous().view(torch.uint8)
        elif valid.dtype not in (torch.float32, torch.uint8):
            raise SdfError(f"augment_chunk: valid is fp32, uint8 or bool, got {valid.dtype}")
        valid = valid.contiguous()
    if drop_u is not None:
        _ptr(drop_u, torch.float32)
        if tuple(drop_u.shape) != (B, bins, h, w) or not drop_u.is_contiguous():
            raise SdfError(f"augment_chunk: drop_u must be a contiguous {(B, bins, h, w)} tensor (output coordinates)")

    def buffer(t, shape, name, wanted=True):
        if not wanted:
            if t is not None:
                raise SdfError(f"augment_chunk: {name} given without its input")
            return None
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise SdfError(f"augment_chunk: {name} must be a contiguous {shape} tensor")
        return t
    out = buffer(out, (B, bins, 2, h, w), "out")
    label_out = buffer(label_out, (B, 2, h, w), "label_out", label is not None)
    mask_out = buffer(mask_out, (B, 1, h, w), "mask_out", valid is not None)
    if event_mask is not None and (tuple(event_mask.shape) != (B, 1, h, w) or not event_mask.is_contiguous()):
        raise SdfError(f"augment_chunk: event_mask must be a contiguous {(B, 1, h, w)} tensor")
    if mask_events and mask_out is None:
        raise SdfError("augment_chunk: mask_events multiplies the valid mask - pass valid")
    need = lib().sdf_augment_chunk_workspace_bytes(B)
    if need <= 0:
        raise SdfError(f"augment_chunk: batch of {B} refused", rc=E_SHAPE)
    ws = _stream_ws(_PC_WS, dev, max(need, 256))
    d = AugmentChunkDesc()
    d.voxel, d.label, d.valid, d.drop_u = voxel.data_ptr(), _ptr(label), _ptr(valid), _ptr(drop_u)
    d.out, d.label_out, d.mask_out = _ptr(out, torch.float32), _ptr(label_out, torch.float32), _ptr(mask_out, torch.float32)
    d.event_mask, d.workspace, d.workspace_bytes = _ptr(event_mask, torch.float32), ws.data_ptr(), ws.numel()
    d.seed, d.offset = (C.c_int64(int(v) & (2 ** 64 - 1)).value for v in (seed, offset))
    d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w = B, bins, Hs, Ws, (h if crop else 0), (w if crop else 0)
    d.valid_is_u8 = int(valid is not None and valid.dtype == torch.uint8)
    d.norm, d.per_sample = {None: 0, "minmax": 1}.get(norm_input, 2), int(bool(per_sample))   # (anything else is the library's to refuse)
    d.use_spike_th, d.spike_th, d.mask_events = int(spike_th is not None), float(spike_th or 0.0), int(bool(mask_events))
    qs = _per_sample("augment_chunk", "drop_q", drop_q, B, 1)
    rows = zip(_per_sample("augment_chunk", "origins", origins, B, 2), _per_sample("augment_chunk", "flips", flips, B, 1), qs)
    for b, ((oy, ox), f, q) in enumerate(rows):
        d.oy[b], d.ox[b], d.flags[b], d.drop_q[b] = int(oy), int(ox), int(f), (-1.0 if q is None else float(q))
    # the window read once (+ drop_u), input / label / mask written once, the finish's read-modify-write of the input
    planes = bins * (3 + (drop_u is not None)) + 4 * (label is not None) + (valid is not None) + 4 * bins * (d.norm == 1 or spike_th is not None)
    _note(bytes=B * h * w * (4 * planes + (valid.element_size() if valid is not None else 0)), shape=(B, bins, 2, h, w))
    _check(lib().sdf_augment_chunk_fwd(C.byref(d), _stream()), "sdf_augment_chunk_fwd")
    return out, label_out, mask_out


def augment_resize_chunk(vox_old, vox_new, flow, crop, params, norm_input="minmax", spike_th=None, per_sample=False, mask_events=False,
                         out=None, label_out=None, mask_out=None, event_mask=None):
    """An MDR loader item -> the training step's (input, label, mask) on the GPU without a host round trip (sdf_augment_resize_fwd): the
    reference's DenseSparseAugmentor (MDR_dataloader.loader_utils) - bilinear rescale, flow * scale, flips, crop, valid mask - then the
    loop's cat((old, new), dim=1), harness.prepare_chunk and, with `mask_events`, mask * event_mask.  vox_old (or None: data.num_chunks
    1) and vox_new (B, bins, Hs, Ws) fp32 signed, flow (B, 2, Hs, Ws) fp32; `crop` (h, w); `params`: one parameter record for every
    sample or a sequence of B (what DenseSparseAugmentor.sample / sample_batch return: resized, scale_x, scale_y, size, hflip, vflip,
    y0, x0).  norm_input / spike_th / per_sample / event_mask as hip.prepare_chunk.  Returns (out (B, nF, 2, h, w) with nF = bins or
    2 bins, old first; label_out (B, 2, h, w); mask_out (B, 1, h, w) fp32); `out`, `label_out`, `mask_out`: contiguous tensors of those
    shapes to write into."""
    _ptr(vox_new, torch.float32)
    if vox_new.dim() != 4:
        raise SdfError(f"augment_resize_chunk: vox_new is (B, bins, H, W), got {tuple(vox_new.shape)}")
    vox_new = vox_new.contiguous()
    B, bins, Hs, Ws = vox_new.shape
    if B > AUGMENT_MAX_B:
        raise SdfError(f"augment_resize_chunk: batch of {B} refused (at most {AUGMENT_MAX_B} per call)", rc=E_SHAPE)
    if vox_old is not None:
        _ptr(vox_old, torch.float32)
        if vox_old.shape != vox_new.shape:
            raise SdfError(f"augment_resize_chunk: vox_old is vox_new's {tuple(vox_new.shape)}, got {tuple(vox_old.shape)}")
        vox_old = vox_old.contiguous()
    _ptr(flow, torch.float32)
    if tuple(flow.shape) != (B, 2, Hs, Ws):
        raise SdfError(f"augment_resize_chunk: flow is {(B, 2, Hs, Ws)}, got {tuple(flow.shape)}")
    flow = flow.contiguous()
    h, w = crop
    nF = bins * (1 + (vox_old is not None))
    dev = vox_new.device

    def buffer(t, shape, name):
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise SdfError(f"augment_resize_chunk: {name} must be a contiguous {shape} tensor")
        return t
    out = buffer(out, (B, nF, 2, h, w), "out")
    label_out = buffer(label_out, (B, 2, h, w), "label_out")
    mask_out = buffer(mask_out, (B, 1, h, w), "mask_out")
    if event_mask is not None and (tuple(event_mask.shape) != (B, 1, h, w) or not event_mask.is_contiguous()):
        raise SdfError(f"augment_resize_chunk: event_mask must be a contiguous {(B, 1, h, w)} tensor")
    rows = [params] * B if not isinstance(params, (list, tuple)) else list(params)
    if len(rows) != B:
        raise SdfError(f"augment_resize_chunk: params is one record or {B} of them (one per sample), got {len(rows)}")
    need = lib().sdf_augment_resize_workspace_bytes(B)
    if need <= 0:
        raise SdfError(f"augment_resize_chunk: batch of {B} refused", rc=E_SHAPE)
    ws = _stream_ws(_PC_WS, dev, max(need, 256))
    d = AugmentResizeDesc()
    sx, sy = ((C.c_double * B)(*(float(getattr(p, k)) for p in rows)) for k in ("scale_x", "scale_y"))
    d.vox_old, d.vox_new, d.flow = _ptr(vox_old), vox_new.data_ptr(), flow.data_ptr()
    d.scale_x, d.scale_y = C.addressof(sx), C.addressof(sy)                # (host arrays, read during the call)
    d.out, d.label_out, d.mask_out = _ptr(out, torch.float32), _ptr(label_out, torch.float32), _ptr(mask_out, torch.float32)
    d.event_mask, d.workspace, d.workspace_bytes = _ptr(event_mask, torch.float32), ws.data_ptr(), ws.numel()
    d.B, d.bins, d.Hs, d.Ws, d.crop_h, d.crop_w, d.num_chunks = B, bins, Hs, Ws, int(h), int(w), 1 + (vox_old is not None)
    d.norm, d.per_sample = {None: 0, "minmax": 1}.get(norm_input, 2), int(bool(per_sample))   # (anything else is the library's to refuse)
    d.use_spike_th, d.spike_th, d.mask_events = int(spike_th is not None), float(spike_th or 0.0), int(bool(mask_events))
    for b, p in enumerate(rows):
        d.resized[b], (d.rh[b], d.rw[b]), d.oy[b], d.ox[b] = int(bool(p.resized)), (int(v) for v in p.size), int(p.y0), int(p.x0)
        d.flags[b] = int(bool(p.hflip)) | int(bool(p.vflip)) << 1
    # four taps (one when not resized) of every plane read, input / label / mask written once, the finish's read-modify-write of the input
    taps = sum(4 if p.resized else 1 for p in rows) / B
    planes = (nF + 2) * taps + 2 * nF + 3 + 4 * nF * (d.norm == 1 or spike_th is not None)
    _note(bytes=int(B * h * w * 4 * planes), shape=(B, nF, 2, h, w))
    _check(lib().sdf_augment_resize_fwd(C.byref(d), _stream()), "sdf_augment_resize_fwd")
    return out, label_out, mask_out


def spike_count_form(spikes, t_dim):
    """(outer, T, rows, C, row_stride) of a u8 tensor or view in sdf_spike_count_fwd's addressing form - element (o, t, r, c) at byte
    ((o T + t) rows + r) row_stride + c behind its first element - with the time steps on dim `t_dim`: 0 (T outermost, outer = 1) or
    1 (a batch in front).  The last dim is the counted run C when it is dense, the dims between it and the step axis must nest into
    ONE row index.  SdfError for everything else (host arithmetic on shapes and strides: no tensor is touched)."""
    if t_dim not in (0, 1) or spikes.dim() <= t_dim:
        raise SdfError(f"spike_count: the step axis is dim 0 or 1 of the tensor, got t_dim {t_dim} for shape {tuple(spikes.shape)}")
    if spikes.numel() == 0:
        raise SdfError(f"spike_count: empty tensor {tuple(spikes.shape)}", rc=E_SHAPE)
    shape, st = list(spikes.shape), list(spikes.stride())
    outer, s_o = (shape[0], st[0]) if t_dim == 1 else (1, 0)
    T, s_t = shape[t_dim], st[t_dim]
    dims = [(n, s) for n, s in zip(shape[t_dim + 1:], st[t_dim + 1:]) if n > 1]
    Cc = dims.pop()[0] if dims and dims[-1][1] == 1 else 1
    rows, rs = 1, None
    for n, s in reversed(dims):
        if rs is None:
            rs = s
        elif s != rows * rs:
            raise SdfError(f"spike_count: shape {tuple(spikes.shape)} with strides {tuple(spikes.stride())} is not (outer, T, rows, C) with "
                           "one row stride; count the parts one by one")
        rows *= n
    if rs is None:                                  # a single row per (o, t): the blocks' own distance is its stride
        rs = s_t if T > 1 else (s_o if outer > 1 else Cc)
    if rs < Cc or (T > 1 and s_t != rows * rs) or (outer > 1 and s_o != T * rows * rs):
        raise SdfError(f"spike_count: shape {tuple(spikes.shape)} with strides {tuple(spikes.stride())} is not (outer, T, rows, C) with "
                       "(o, t) blocks rows x row stride apart; count the parts one by one")
    return outer, T, rows, Cc, rs


def spike_count(spikes, t_dim, counts=None):
    """Spikes per time step of a u8 tensor or view (sdf_spike_count_fwd): counts[t] += the sum over everything but dim `t_dim` (0, or
    1 behind a batch dim).  `counts`: a contiguous int64 tensor of T entries on the same device that is ADDED to (default: a new,
    zeroed one).  Views are counted in place - channel slices, halves of a stacked buffer, slices of a workspace (spike_count_form);
    there is no .contiguous() and no torch fallback: a layout outside that form raises SdfError."""
    if not torch.is_tensor(spikes) or not spikes.is_cuda:
        raise SdfError("spike_count: HIP path needs a device tensor (no CPU fallback)")
    if spikes.dtype != torch.uint8:
        raise SdfError(f"spike_count: spikes are u8, got {spikes.dtype}", rc=E_DTYPE)
    outer, T, rows, Cc, rs = spike_count_form(spikes, t_dim)
    if counts is None:
        counts = torch.zeros(T, dtype=torch.int64, device=spikes.device)
    elif not (torch.is_tensor(counts) and counts.is_cuda and counts.device == spikes.device and counts.dtype == torch.int64
              and counts.dim() == 1 and counts.numel() == T and counts.is_contiguous()):
        raise SdfError(f"spike_count: counts must be a contiguous int64 tensor of T = {T} entries on {spikes.device}")
    d = SpikeCountDesc()
    d.spikes, d.counts = spikes.data_ptr(), counts.data_ptr()
    d.outer, d.T, d.rows, d.C, d.row_stride = outer, T, rows, Cc, rs
    _note(bytes=outer * T * rows * Cc, shape=(outer, T, rows, Cc))
    _check(lib().sdf_spike_count_fwd(C.byref(d), _stream()), "sdf_spike_count_fwd")
    return counts


def spike_count_samples_form(spikes, t_dim, samples):
    """(s_out, T, s_in, rows, C, row_stride) of a u8 tensor or view that holds `samples` independent samples, in
    sdf_spike_count_seg_fwd's addressing form - element (so, t, si, r, c) at byte (((so T + t) s_in + si) rows + r) row_stride + c behind
    its first element.  t_dim 1: the samples are dim 0, outside time (s_in = 1; channel-last (B, D, h, w, C) records and their channel
    slices).  t_dim 0: the samples are `samples` equal consecutive pieces of every time block (s_out = 1; the window records of a replica
    forward): the rows of a block must divide by `samples`.  Everything else is spike_count_form's, its refusals included; host
    arithmetic on shapes and strides, no tensor is touched."""
    if not torch.is_tensor(spikes) or spikes.dtype != torch.uint8:
        raise SdfError(f"spike_count_samples: spikes are a u8 tensor, got {getattr(spikes, 'dtype', type(spikes).__name__)}", rc=E_DTYPE)
    samples = int(samples)
    if samples < 1:
        raise SdfError(f"spike_count_samples: {samples} samples", rc=E_SHAPE)
    outer, T, rows, Cc, rs = spike_count_form(spikes, t_dim)
    if t_dim == 1:
        if outer != samples:
            raise SdfError(f"spike_count_samples: the step axis is dim 1, so the samples are dim 0: shape {tuple(spikes.shape)} holds "
                           f"{outer}, not {samples} (one count over a batch is spike_count's)", rc=E_SHAPE)
        return outer, T, 1, rows, Cc, rs
    if rows % samples:
        raise SdfError(f"spike_count_samples: the {rows} rows of a time block of shape {tuple(spikes.shape)} do not split into {samples} "
                       "equal consecutive pieces", rc=E_SHAPE)
    return 1, T, samples, rows // samples, Cc, rs


def spike_count_samples(spikes, t_dim, samples, counts):
    """Spikes per SAMPLE and time step of a u8 tensor or view (sdf_spike_count_seg_fwd): counts[s, t] += the sum over sample s's bytes of
    step t (spike_count_samples_form says where they lie).  `counts`: an int64 view (samples, T) on the same device, dense along T, its
    rows any distance >= T apart - e.g. block[:, call, :T] of a (samples, calls, Tmax) block - that is ADDED to.  One launch, counted in
    place, no torch fallback."""
    if not torch.is_tensor(spikes) or not spikes.is_cuda:
        raise SdfError("spike_count_samples: HIP path needs a device tensor (no CPU fallback)")
    s_out, T, s_in, rows, Cc, rs = spike_count_samples_form(spikes, t_dim, samples)
    n = s_out * s_in
    if not (torch.is_tensor(counts) and counts.is_cuda and counts.device == spikes.device and counts.dtype == torch.int64
            and tuple(counts.shape) == (n, T) and (T == 1 or counts.stride(1) == 1) and (n == 1 or counts.stride(0) >= T)):
        raise SdfError(f"spike_count_samples: counts must be an int64 view ({n}, {T}) on {spikes.device}, dense along the steps, its "
                       f"rows at least {T} apart")
    d = SpikeCountSegDesc()
    d.spikes, d.counts = spikes.data_ptr(), counts.data_ptr()
    d.s_out, d.T, d.s_in, d.rows, d.C, d.row_stride = s_out, T, s_in, rows, Cc, rs
    d.sample_pitch = counts.stride(0) if n > 1 else T
    _note(bytes=n * T * rows * Cc, shape=(s_out, T, s_in, rows, Cc))
    _check(lib().sdf_spike_count_seg_fwd(C.byref(d), _stream()), "sdf_spike_count_seg_fwd")
    return counts


MEMBRANE_HEAD = 4                                   # [n_nan, sum_q16, min_key, max_key] in front of a record's histogram
MEMBRANE_KEY_INIT = (0xFFFFFFFF, 0)                 # what the caller puts into min_key / max_key before the first call


def membrane_inv_width(lo, hi, bins):
    """(lo, hi, inv_width) as sdf_membrane_stats_fwd takes them: fp32 bounds and bins / (hi - lo) formed ONCE in fp32 on the host."""
    lo32, hi32 = torch.tensor(float(lo), dtype=torch.float32), torch.tensor(float(hi), dtype=torch.float32)
    return lo32.item(), hi32.item(), (torch.tensor(float(bins), dtype=torch.float32) / (hi32 - lo32)).item()


def membrane_table(T, bins, device):
    """A fresh (T, 4 + bins + 2) int64 record table: zeros, min_key = 2^32 - 1, max_key = 0."""
    table = torch.zeros((T, MEMBRANE_HEAD + bins + 2), dtype=torch.int64, device=device)
    table[:, 2] = MEMBRANE_KEY_INIT[0]
    return table


def membrane_stats(v, t_dim, table=None, lo=-2.0, hi=2.0, bins=64):
    """Per-step statistics of an fp32 membrane tensor or view (sdf_membrane_stats_fwd): record t of `table` - (T, 4 + bins + 2) int64,
    contiguous, same device - takes [n_nan, sum_q16, min_key, max_key, hist] over everything but dim `t_dim` (0, or 1 behind a batch
    dim) and is ADDED to (default: a fresh membrane_table).  Views are read in place (spike_count_form's addressing, in elements);
    there is no .contiguous() and no torch fallback: a layout outside that form raises SdfError."""
    if not torch.is_tensor(v) or not v.is_cuda:
        raise SdfError("membrane_stats: HIP path needs a device tensor (no CPU fallback)")
    if v.dtype != torch.float32:
        raise SdfError(f"membrane_stats: membranes are fp32, got {v.dtype}", rc=E_DTYPE)
    bins = int(bins)
    if not 1 <= bins <= 256:
        raise SdfError(f"membrane_stats: {bins} bins; the kernel's LDS histogram takes 1 to 256", rc=E_SHAPE)
    outer, T, rows, Cc, rs = spike_count_form(v, t_dim)
    if table is None:
        table = membrane_table(T, bins, v.device)
    elif not (torch.is_tensor(table) and table.is_cuda and table.device == v.device and table.dtype == torch.int64
              and tuple(table.shape) == (T, MEMBRANE_HEAD + bins + 2) and table.is_contiguous()):
        raise SdfError(f"membrane_stats: table must be a contiguous int64 tensor of shape ({T}, {MEMBRANE_HEAD + bins + 2}) on {v.device}")
    d = MembraneStatsDesc()
    d.v, d.table = v.data_ptr(), table.data_ptr()
    d.outer, d.T, d.rows, d.C, d.row_stride, d.bins = outer, T, rows, Cc, rs, bins
    d.lo, d.hi, d.inv_width = membrane_inv_width(lo, hi, bins)
    _note(bytes=outer * T * rows * Cc * 4, shape=(outer, T, rows, Cc))
    _check(lib().sdf_membrane_stats_fwd(C.byref(d), _stream()), "sdf_membrane_stats_fwd")
    return table


GRAD_STATS_FIELDS = ("sum_abs", "sum_sq", "min_abs", "max_abs", "nonfinite")
_GS_WS = {}


class GradSegments:
    """The parameters of one flat fp32 buffer as the grad-step entry points take them: (offset, length) pairs in floats, ascending and
    not overlapping, once on the host (the entry points' checks) and once on `device` (the kernels)."""

    def __init__(self, pairs, device):
        import numpy as np
        self.host = np.ascontiguousarray(np.asarray(list(pairs), dtype=np.int64).reshape(-1, 2))
        self.n = int(self.host.shape[0])
        self.dev = torch.from_numpy(self.host).to(device)


def adamw_rows(n):
    """A host table of n SdfAdamwRow as a numpy structured array (fill it by field; `hip.adamw_step` takes it as it is)."""
    import numpy as np
    dt = np.dtype([("param", np.uint64), ("offset", np.int64), ("length", np.int64), ("decay", np.float32), ("w1", np.float32),
                   ("beta2", np.float32), ("w2", np.float32), ("neg_step_size", np.float32), ("bc2_sqrt", np.float32),
                   ("eps", np.float32), ("active", np.int32)], align=True)
    assert dt.itemsize == C.sizeof(AdamwRow) and all(dt.fields[f][1] == getattr(AdamwRow, f).offset for f, _ in AdamwRow._fields_)
    return np.zeros(n, dtype=dt)


def _flat_f32(fn, name, t):
    _ptr(t, torch.float32)
    if t.dim() != 1 or not t.is_contiguous():
        raise SdfError(f"{fn}: {name} is a flat contiguous fp32 tensor, got {tuple(t.shape)}")
    return t


def grad_stats(flat, segments, table=None, row=0):
    """Per-parameter gradient statistics of a flat fp32 bucket on the GPU (sdf_grad_stats_fwd: two launches, no read-back, no float
    atomics): segment s of `segments` - a GradSegments, or (offset, length) pairs - writes row `row` + s of `table` (rows, 5) float64 -
    GRAD_STATS_FIELDS: sum |g|, sum g^2, min |g|, max |g| over the finite elements (fp64, both terms exact) and the count of the
    others - and leaves the other rows as they are.  `table` None: a new zero table of row + n rows.  Returns the table.  Identical
    bytes from run to run."""
    _flat_f32("grad_stats", "flat", flat)
    dev = flat.device
    if not isinstance(segments, GradSegments):
        segments = GradSegments(segments, dev)
    table = _record_table("grad_stats", table, row, segments.n, GRAD_STATS_FIELDS, dev)
    need = lib().sdf_grad_stats_workspace_bytes(segments.n)
    if need <= 0:
        raise SdfError(f"grad_stats: {segments.n} segments; the entry point takes 1 to 65535", rc=E_SHAPE)
    ws = _stream_ws(_GS_WS, dev, need)
    d = GradStatsDesc()
    d.flat, d.n, d.seg_host, d.seg, d.nseg = flat.data_ptr(), flat.numel(), segments.host.ctypes.data, segments.dev.data_ptr(), segments.n
    d.row0, d.rows, d.table, d.workspace, d.workspace_bytes = row, table.shape[0], table.data_ptr(), ws.data_ptr(), ws.numel()
    _check(lib().sdf_grad_stats_fwd(C.byref(d), _stream()), "sdf_grad_stats_fwd")
    return table


def grad_clip_coef(table, max_norm, mask=None, coef=None, record=None):
    """torch.nn.utils.clip_grad_norm_'s coefficient from a grad_stats table, on the GPU (sdf_grad_clip_coef: one launch, no read-back):
    total = sqrt(sum of sum_sq over the rows with mask != 0 (`mask`: (rows,) uint8 or None: all)) in fp64, coef = min(1, max_norm /
    (total + 1e-6)) as one fp32.  max_norm is taken as fp32; inf gives coef 1.  Returns (coef (1,) float32, record (2,) float64 =
    [total, non-finite count]), both device tensors - `coef` / `record` when given."""
    _ptr(table, torch.float64)
    if table.dim() != 2 or table.shape[1] != len(GRAD_STATS_FIELDS) or not table.is_contiguous():
        raise SdfError(f"grad_clip_coef: table must be a contiguous (rows, {len(GRAD_STATS_FIELDS)}) float64 tensor")
    dev = table.device
    if mask is not None and (_ptr(mask, torch.uint8) is None or mask.shape != (table.shape[0],) or not mask.is_contiguous()):
        raise SdfError(f"grad_clip_coef: mask is a contiguous ({table.shape[0]},) uint8 tensor")
    coef = torch.empty(1, dtype=torch.float32, device=dev) if coef is None else coef
    record = torch.empty(2, dtype=torch.float64, device=dev) if record is None else record
    if coef.numel() != 1 or record.numel() != 2:
        raise SdfError("grad_clip_coef: coef holds one float32 and record two float64")
    _check(lib().sdf_grad_clip_coef(table.data_ptr(), table.shape[0], _ptr(mask), float(max_norm), _ptr(coef, torch.float32),
                                    _ptr(record, torch.float64), _stream()), "sdf_grad_clip_coef")
    return coef, record


def adamw_step(grad, exp_avg, exp_avg_sq, rows, rows_dev=None, coef=None):
    """torch.optim.AdamW(foreach=False)'s update of the parameters of one flat bucket (sdf_adamw_step: one launch; one read of g, m, v, p
    and one write of m, v, p): `rows` is an adamw_rows() table - per parameter its data pointer, its segment of the three flat
    buffers, the step's scalars and `active` (0: nothing of it is touched); `rows_dev` the same bytes on the device (None: copied
    here, which waits for the copy).  `coef` (1,) float32 on the device multiplies every gradient as it is read (grad_clip_coef).
    The parameters are written through their raw pointers: the CALLER moves their version counters."""
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _flat_f32("adamw_step", name, t)
    if exp_avg.numel() != grad.numel() or exp_avg_sq.numel() != grad.numel():
        raise SdfError("adamw_step: the moments mirror the gradient bucket")
    if rows.dtype.itemsize != C.sizeof(AdamwRow) or not rows.flags["C_CONTIGUOUS"]:
        raise SdfError("adamw_step: rows is an adamw_rows() table")
    if rows_dev is None:
        rows_dev = torch.from_numpy(rows.view("uint8")).to(grad.device)
    if _ptr(rows_dev, torch.uint8) is None or rows_dev.numel() < rows.nbytes or not rows_dev.is_contiguous():
        raise SdfError("adamw_step: rows_dev holds the bytes of rows on the device")
    d = AdamwDesc()
    d.grad, d.exp_avg, d.exp_avg_sq, d.n = grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.numel()
    d.rows_host, d.rows, d.nseg, d.coef = rows.ctypes.data, rows_dev.data_ptr(), len(rows), _ptr(coef, torch.float32)
    _note(bytes=int(rows["length"][rows["active"] != 0].sum()) * 28)
    _check(lib().sdf_adamw_step(C.byref(d), _stream()), "sdf_adamw_step")


def loss_scale_state(scale=65536.0, growth_tracker=0, device="cuda"):
    """A SdfLossScaleState in device memory as a (3,) int64 tensor (24 bytes, 8-byte aligned): scale, growth_tracker, inv_scale = 1 /
    scale, found_inf = 0, skipped = 0.  `loss_scale_views(state)` names its members."""
    import numpy as np
    host = np.zeros(1, dtype=loss_scale_dtype())
    host["scale"], host["growth_tracker"] = scale, growth_tracker
    host["inv_scale"] = np.float32(1.0 / np.float64(host["scale"][0]))
    return torch.from_numpy(host.view(np.int64).copy()).to(device)


def loss_scale_dtype():
    """SdfLossScaleState as a numpy structured dtype."""
    import numpy as np
    dt = np.dtype([("scale", np.float32), ("growth_tracker", np.int32), ("inv_scale", np.float32), ("found_inf", np.int32),
                   ("skipped", np.int64)], align=True)
    assert dt.itemsize == C.sizeof(LossScaleState) and all(dt.fields[f][1] == getattr(LossScaleState, f).offset for f, _ in LossScaleState._fields_)
    return dt


def loss_scale_views(state):
    """{member: one-element view} of a loss_scale_state tensor: scale / inv_scale float32, growth_tracker / found_inf int32, skipped int64."""
    f, i = state.view(torch.float32), state.view(torch.int32)
    return {"scale": f[0:1], "growth_tracker": i[1:2], "inv_scale": f[2:3], "found_inf": i[3:4], "skipped": state[2:3]}


def loss_scale_read(state):
    """One read-back of a loss_scale_state: {member: Python number}."""
    host = state.cpu().numpy().view(loss_scale_dtype())[0]
    return {k: host[k].item() for k in host.dtype.names}


def _loss_scale_ptr(fn, state):
    if not (torch.is_tensor(state) and state.dtype == torch.int64 and state.numel() == 3 and state.is_contiguous()):
        raise SdfError(f"{fn}: state is a hip.loss_scale_state() tensor")
    return _ptr(state, torch.int64)


def grad_scale(flat, segments, coef, mask=None):
    """flat[segment] *= coef[0] in place over every segment of a flat fp32 bucket whose mask byte is non-zero (sdf_grad_scale_inplace:
    one launch; `coef` (1,) float32 and `mask` (n segments,) uint8 on the device, mask None: every segment) - what clip_grad_norm_
    does to a running sum of gradients, the coefficient never leaving the device.  Nothing outside an active segment is touched."""
    _flat_f32("grad_scale", "flat", flat)
    if not isinstance(segments, GradSegments):
        segments = GradSegments(segments, flat.device)
    if _ptr(coef, torch.float32) is None or coef.numel() != 1:
        raise SdfError("grad_scale: coef holds one float32 on the device")
    if mask is not None and (_ptr(mask, torch.uint8) is None or mask.shape != (segments.n,) or not mask.is_contiguous()):
        raise SdfError(f"grad_scale: mask is a contiguous ({segments.n},) uint8 tensor")
    d = GradScaleDesc()
    d.flat, d.n, d.seg_host, d.seg, d.nseg = flat.data_ptr(), flat.numel(), segments.host.ctypes.data, segments.dev.data_ptr(), segments.n
    d.mask, d.coef = _ptr(mask), coef.data_ptr()
    _note(bytes=int(segments.host[:, 1].sum()) * 8)
    _check(lib().sdf_grad_scale_inplace(C.byref(d), _stream()), "sdf_grad_scale_inplace")
    return flat


def grad_clip_scale_coef(table, max_norm, state, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, mask=None, coef=None,
                         record=None, clip_unscaled=False, update=True):
    """grad_clip_coef and the loss scaler in one launch of one workgroup (sdf_grad_clip_scale_coef): coef and record as grad_clip_coef
    gives them - with `clip_unscaled` the norm is divided by the scale first, the textbook order - and in `state`
    (hip.loss_scale_state) found_inf = a non-finite gradient was counted, inv_scale = 1 / the scale these gradients carry, skipped +=
    found_inf, and then torch's _amp_update_scale_ with the two factors taken as fp32 (`update` False: scale and tracker stay).
    Returns (coef, record)."""
    _ptr(table, torch.float64)
    if table.dim() != 2 or table.shape[1] != len(GRAD_STATS_FIELDS) or not table.is_contiguous():
        raise SdfError(f"grad_clip_scale_coef: table must be a contiguous (rows, {len(GRAD_STATS_FIELDS)}) float64 tensor")
    dev = table.device
    if mask is not None and (_ptr(mask, torch.uint8) is None or mask.shape != (table.shape[0],) or not mask.is_contiguous()):
        raise SdfError(f"grad_clip_scale_coef: mask is a contiguous ({table.shape[0]},) uint8 tensor")
    coef = torch.empty(1, dtype=torch.float32, device=dev) if coef is None else coef
    record = torch.empty(2, dtype=torch.float64, device=dev) if record is None else record
    if coef.numel() != 1 or record.numel() != 2:
        raise SdfError("grad_clip_scale_coef: coef holds one float32 and record two float64")
    d = GradClipScaleDesc()
    d.table, d.rows, d.mask, d.max_norm = table.data_ptr(), table.shape[0], _ptr(mask), float(max_norm)
    d.coef, d.record, d.state = _ptr(coef, torch.float32), _ptr(record, torch.float64), _loss_scale_ptr("grad_clip_scale_coef", state)
    d.growth_factor, d.backoff_factor, d.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
    d.clip_unscaled, d.update = int(bool(clip_unscaled)), int(bool(update))
    _check(lib().sdf_grad_clip_scale_coef(C.byref(d), _stream()), "sdf_grad_clip_scale_coef")
    return coef, record


def adamw_step_scaled(grad, exp_avg, exp_avg_sq, rows, state, rows_dev=None, coef=None):
    """adamw_step under a loss scaler (sdf_adamw_step_scaled: one launch): with state.found_inf set no parameter and no moment is
    written; otherwise the update runs on (grad * coef) * state.inv_scale.  `state`: hip.loss_scale_state, as grad_clip_scale_coef
    left it.  The other arguments are adamw_step's."""
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        _flat_f32("adamw_step_scaled", name, t)
    if exp_avg.numel() != grad.numel() or exp_avg_sq.numel() != grad.numel():
        raise SdfError("adamw_step_scaled: the moments mirror the gradient bucket")
    if rows.dtype.itemsize != C.sizeof(AdamwRow) or not rows.flags["C_CONTIGUOUS"]:
        raise SdfError("adamw_step_scaled: rows is an adamw_rows() table")
    sp = _loss_scale_ptr("adamw_step_scaled", state)
    if rows_dev is None:
        rows_dev = torch.from_numpy(rows.view("uint8")).to(grad.device)
    if _ptr(rows_dev, torch.uint8) is None or rows_dev.numel() < rows.nbytes or not rows_dev.is_contiguous():
        raise SdfError("adamw_step_scaled: rows_dev holds the bytes of rows on the device")
    d = AdamwDesc()
    d.grad, d.exp_avg, d.exp_avg_sq, d.n = grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), grad.numel()
    d.rows_host, d.rows, d.nseg, d.coef = rows.ctypes.data, rows_dev.data_ptr(), len(rows), _ptr(coef, torch.float32)
    _note(bytes=int(rows["length"][rows["active"] != 0].sum()) * 28)
    _check(lib().sdf_adamw_step_scaled(C.byref(d), C.cast(C.c_void_p(sp), C.POINTER(LossScaleState)), _stream()), "sdf_adamw_step_scaled")


_FI_WS, _EI_Q = {}, {}


def _flow_planes(fn, flow):
    """(flow contiguous, B, H, W) of a (B, 2, H, W) fp32 device tensor (`fn` prefixes the message)."""
    _ptr(flow, torch.float32)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise SdfError(f"{fn}: flow is (B, 2, H, W), got {tuple(flow.shape)}")
    return (flow.contiguous(),) + tuple(flow.shape[0:1] + flow.shape[2:])


def _image_out(fn, out, shape, dtype, dev):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()):
        raise SdfError(f"{fn}: out must be a contiguous {shape} {dtype} tensor on {dev}")
    return out


def flow_image(flow, mask=None, out=None):
    """The reference's Visualization_DSEC.flow_to_image of every sample on the GPU (sdf_flow_image_fwd: two launches, no read-back,
    nothing allocated when `out` is given): flow (B, 2, H, W) fp32 [* mask (B, 1, H, W) or (B, H, W) fp32] -> (B, H, W, 3) u8 RGB.
    Hue = direction, value = magnitude scaled by the SAMPLE's own min / max (a sample's bytes do not depend on its batch); identical
    bytes from run to run.  NaN flows give unspecified bytes."""
    flow, B, H, W = _flow_planes("flow_image", flow)
    dev = flow.device
    if mask is not None:
        _ptr(mask, torch.float32)
        if mask.numel() != B * H * W or tuple(mask.shape[-2:]) != (H, W):
            raise SdfError(f"flow_image: mask is (B, 1, H, W) or (B, H, W) at the flow's size, got {tuple(mask.shape)}")
        mask = mask.contiguous()
    out = _image_out("flow_image", out, (B, H, W, 3), torch.uint8, dev)
    need = lib().sdf_flow_image_workspace_bytes(B, H, W)
    if need <= 0:
        raise SdfError(f"flow_image: geometry refused (B {B}, {H} x {W})", rc=E_SHAPE)
    ws = _stream_ws(_FI_WS, dev, max(need, 256))
    d = FlowImageDesc()
    d.flow, d.mask, d.out = flow.data_ptr(), _ptr(mask, torch.float32), out.data_ptr()
    d.workspace, d.workspace_bytes, d.B, d.H, d.W = ws.data_ptr(), ws.numel(), B, H, W
    _note(bytes=B * H * W * (2 * (8 + 4 * (mask is not None)) + 3), shape=(B, H, W))
    _check(lib().sdf_flow_image_fwd(C.byref(d), _stream()), "sdf_flow_image_fwd")
    return out


def flow_submission(flow, out=None):
    """Flow maps in the DSEC benchmark's 16-bit encoding on the GPU (sdf_flow_submission_fwd, the reference's `flow_test` branch of
    Visualization_DSEC.store): flow (B, 2, H, W) fp32 -> (B, H, W, 3) uint16, channels 0 / 1 = (uint16)(f * 128 + 2 ** 15) in fp32,
    channel 2 = 0.  Bit-exact for |f| < 256 px.  Beyond that the reference's numpy cast is undefined; here the value CLAMPS to
    [0, 65535] (NaN: 0)."""
    flow, B, H, W = _flow_planes("flow_submission", flow)
    out = _image_out("flow_submission", out, (B, H, W, 3), torch.uint16, flow.device)
    d = FlowSubmissionDesc()
    d.flow, d.out, d.B, d.H, d.W = flow.data_ptr(), out.data_ptr(), B, H, W
    _note(bytes=B * H * W * (8 + 6), shape=(B, H, W))
    _check(lib().sdf_flow_submission_fwd(C.byref(d), _stream()), "sdf_flow_submission_fwd")
    return out


def event_counts(voxel_or_input, crop=None, crop_origin=None, out=None):
    """The loops' `chunk_vis` on the GPU (stage 0 of sdf_event_image_fwd): per pixel the positive and the negative event sums over the
    bins, added in bin order -> (B, 2, h, w) fp32.  A 4-D tensor is a signed voxel (B, bins, Hs, Ws) ("signed" mode: sums of relu(v) /
    relu(-v), eval_DSEC_flow_SNN.py:182-188); a 5-D one is the model's input (B, bins, 2, Hs, Ws) ("split" mode: channels 0 / 1
    summed).  `crop` (h, w) at `crop_origin` (default harness.center_crop's)."""
    src = voxel_or_input
    _ptr(src, torch.float32)
    if src.dim() not in (4, 5) or (src.dim() == 5 and src.shape[2] != 2):
        raise SdfError(f"event_counts: a signed voxel (B, bins, H, W) or the model's input (B, bins, 2, H, W), got {tuple(src.shape)}")
    src = src.contiguous()
    B, bins, (Hs, Ws) = src.shape[0], src.shape[1], src.shape[-2:]
    h, w = crop if crop else (Hs, Ws)
    oy, ox = crop_origin if crop_origin is not None else (((Hs - h) // 2, (Ws - w) // 2) if crop else (0, 0))
    if out is None:
        out = torch.empty((B, 2, h, w), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (B, 2, h, w) or not out.is_contiguous():
        raise SdfError(f"event_counts: out must be a contiguous {(B, 2, h, w)} tensor")
    d = EventImageDesc()
    d.src, d.chunk_vis = src.data_ptr(), _ptr(out, torch.float32)
    d.B, d.bins, d.Hs, d.Ws = B, bins, Hs, Ws
    d.crop_h, d.crop_w, d.crop_oy, d.crop_ox = (h if crop else 0), (w if crop else 0), oy, ox
    d.mode, d.stage = int(src.dim() == 5), 0
    _note(bytes=B * bins * h * w * 4 + B * h * w * 8, shape=(B, bins, h, w))
    _check(lib().sdf_event_image_fwd(C.byref(d), _stream()), "sdf_event_image_fwd")
    return out


def event_image(voxel_or_input, crop=None, crop_origin=None, out=None):
    """The stored event image of every sample on the GPU: event_counts (the loops' `chunk_vis`) rendered as the reference's
    events_to_image (green_red) and byte-ordered as cv2.imwrite stores it: (B, h, w, 3) u8 RGB = (neg', pos', 0), each polarity scaled
    between its 1st percentile and the larger 99th percentile of the two, per sample.  Stage 0 of sdf_event_image_fwd |
    torch.quantile on the stream (linear interpolation, numpy's default) | stage 1; no read-back.  The byte is rint(255 x) with halves
    to even - OpenCV's documented saturate_cast, not checked against cv2 itself."""
    return event_counts_image(event_counts(voxel_or_input, crop, crop_origin), out=out)


def event_counts_image(counts, out=None):
    """event_image's second half on its own: counts (B, 2, h, w) fp32 - a sample's positive and negative event sums, the loops'
    `chunk_vis` - -> (B, h, w, 3) u8 RGB as stored (percentiles by torch.quantile on the stream, then stage 1 of sdf_event_image_fwd)."""
    _ptr(counts, torch.float32)
    if counts.dim() != 4 or counts.shape[1] != 2:
        raise SdfError(f"event_counts_image: counts are (B, 2, h, w), got {tuple(counts.shape)}")
    vis = counts.contiguous()
    B, _, h, w = vis.shape
    dev = vis.device
    out = _image_out("event_counts_image", out, (B, h, w, 3), torch.uint8, dev)
    if str(dev) not in _EI_Q:
        _EI_Q[str(dev)] = torch.tensor([0.01, 0.99], dtype=torch.float32, device=dev)
    # plumbing: (2, B * 2) percentiles [q][sample, polarity] -> (B, 4) {pos_min, pos_max, neg_min, neg_max}
    bounds = torch.quantile(vis.view(B * 2, h * w), _EI_Q[str(dev)], dim=1).view(2, B, 2).permute(1, 2, 0).reshape(B, 4).contiguous()
    d = EventImageDesc()
    d.chunk_vis, d.bounds, d.out = vis.data_ptr(), bounds.data_ptr(), out.data_ptr()
    d.B, d.bins, d.Hs, d.Ws, d.stage = B, 1, h, w, 1
    _note(bytes=B * h * w * (8 + 3), shape=(B, h, w))
    _check(lib().sdf_event_image_fwd(C.byref(d), _stream()), "sdf_event_image_fwd")
    return out
