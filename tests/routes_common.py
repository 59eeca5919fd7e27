"""Shared by the launch-list pins (test_digit_routes_gpu.py, test_stage0_routes_gpu.py): random operands, the neurons of the three
compile-time classes, and one call's launches read from hip.launch_log() as "workgroups threads LDS-bytes kernel<template arguments>"."""
import re

import torch

from sdformerflow_amd import hip

DEV = "cuda:0"


def rnd(shape, lo=-0.1, hi=0.1):
    return torch.rand(shape, device=DEV) * (hi - lo) + lo


def neuron(name, T):
    """class 0: LIF with a soft reset; class 1: PSN (its own T x T matrix); class 2: hard reset, IF"""
    if name == "psn":
        return hip.NeuronParams("psn", psn_w=(torch.eye(T, device=DEV) * 0.8).contiguous(), psn_b=torch.full((T,), -0.1, device=DEV))
    return {"lif": hip.NeuronParams("lif", 2.0, 0.1, None), "lif_hard": hip.NeuronParams("lif", 2.0, 0.1, 0.0),
            "if": hip.NeuronParams("if", 2.0, 0.1, None)}[name]


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\b(sdfmm|sdf)::", "", name)
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    return re.sub(r"\(.*$", "", name)


def logged(call):
    """(the launches of one call, what it returned); a call the library refuses ends its list with "rc <code>" and returns ()"""
    out, rc = (), None
    with hip.launch_log() as log:
        try:
            out = call()
        except hip.SdfError as e:
            rc = e.rc
    torch.cuda.synchronize()
    return [f"{wgs} {thr} {lds} {short(k)}" for k, wgs, thr, lds, _ in log.rows] + ([f"rc {rc}"] if rc is not None else []), out
