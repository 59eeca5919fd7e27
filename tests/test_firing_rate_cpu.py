"""Host-side checks of the firing-rate monitor (no GPU): its call list is the reference's, in the reference's order, for both model
families (the names the fixtures recorded on the reference's own forward), and what it refuses it refuses before touching a device."""
import os

import numpy as np
import pytest
import torch
import yaml

from sdformerflow_amd import harness, hip
from sdformerflow_amd.monitor import FiringRateMonitor, neuron_call_names
from sdformerflow_amd.STSwinNet_SNN.Spiking_STSwinNet import MS_SpikingformerFlowNet, MS_SpikingformerFlowNet_en4, SpikingformerFlowNet

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "..", "sdformerflow_amd", "configs", "train_DSEC_supervised_SDformerFlow_en4.yml")
EN3 = dict(swin_depths=[2, 2, 6], swin_num_heads=[3, 6, 12], swin_out_indices=[0, 1, 2])


def build(cls, kind, size, en3):
    cfg = yaml.safe_load(open(CFG))
    cfg["model"]["spiking_neuron"] = dict(cfg["spiking_neuron"], neuron_type=kind)
    cfg["swin_transformer"].update(input_size=list(size), window_size=[2, 9, 9], **(EN3 if en3 else {}))
    return cls(cfg["model"].copy(), cfg["swin_transformer"].copy()), cfg


@pytest.mark.parametrize("kind", ["lif", "psn"])
def test_call_names_are_the_reference_calls_in_order(kind):
    g = np.load(os.path.join(HERE, "golden", "end_to_end.npz"))
    model, _ = build(MS_SpikingformerFlowNet_en4, kind, (288, 384), False)
    names = neuron_call_names(model)
    assert names == [str(n) for n in g[f"{kind}_rate_names"]] and len(names) == 105
    assert FiringRateMonitor(model).names == names
    # every name is a module of the tree (the state_dict prefix of a Spiking_neuron's neuron, without the trailing dot)
    modules = dict(model.named_modules())
    assert all(n in modules for n in names)
    g = np.load(os.path.join(HERE, "golden", "sew_end_to_end.npz"))
    sew, _ = build(SpikingformerFlowNet, kind, (144, 192), True)
    names = neuron_call_names(sew)
    assert names == [str(n) for n in g[f"{kind}_rate_names"]] and len(names) == 75
    assert all(n in dict(sew.named_modules()) for n in names)


def test_monitor_switching_and_host_side_refusals():
    model, cfg = build(MS_SpikingformerFlowNet, "lif", (144, 192), True)
    model.eval()
    mon = FiringRateMonitor(model)
    assert mon.Tmax == 10 and not mon.enabled and mon.forwards == 0 and mon.records == [] and mon.elements == []
    assert mon.mean() != mon.mean()                                            # NaN: nothing recorded
    with mon:
        assert mon.enabled and model._fr_monitor is mon
        with pytest.raises(RuntimeError, match="another FiringRateMonitor"):
            FiringRateMonitor(model).enable()
        with pytest.raises(hip.SdfError):                                      # no CPU fallback, monitored or not
            model(torch.zeros(1, 10, 2, 144, 192))
        with pytest.raises(RuntimeError, match="forward_replicas"):
            model.forward_replicas(torch.zeros(2, 10, 2, 144, 192))
    assert not mon.enabled and model._fr_monitor is None and mon.forwards == 0
    mon.enable().disable()
    assert model._fr_monitor is None
    # the throughput scheme refuses the key before it creates a stream
    cfg["metrics"] = {"mask_events": False, "flow_scaling": 1}
    cfg["vis"] = {"monitor_fr": True}
    # a monitor of another model would record nothing: refused before the loop starts
    other, _ = build(MS_SpikingformerFlowNet, "lif", (144, 192), True)
    with pytest.raises(ValueError, match="another model"):
        harness.evaluate(model, [], cfg, device="cpu", monitor=FiringRateMonitor(other))
    assert mon.counts().shape == (0, len(mon.names), 10) and mon.counts().device.type == "cpu"      # empty: where the model lies
    with pytest.raises(RuntimeError, match="monitor_fr"):
        harness.evaluate_stream(model, [], cfg)
    # the ANN model has no neuron calls
    from sdformerflow_amd.STSwinNet.STSwinNet import STTFlowNet
    with pytest.raises(hip.SdfError, match="spiking model"):
        FiringRateMonitor(STTFlowNet.__new__(STTFlowNet))
