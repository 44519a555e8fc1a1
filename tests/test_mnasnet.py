"""MNASNet: torchvision-compatible layout, registry entries, CPU paths."""
import pytest
import torch
import torch.nn.functional as F

from amdtrain.config import base_parser
from amdtrain.models import MNASNet, build_model, model_names
from amdtrain.ops.conv import AmdConv2d, dwconv5x5


@pytest.fixture(scope="module")
def net1000():
    return build_model("mnasnet1_0")


def test_param_counts(net1000):
    assert isinstance(net1000, MNASNet)
    assert sum(p.numel() for p in net1000.parameters()) == 4_383_312
    half = build_model("mnasnet0_5")
    assert sum(p.numel() for p in half.parameters()) == 2_218_512


def test_state_dict_layout(net1000):
    sd = net1000.state_dict()
    assert len(sd) == 314
    for k in ["layers.1.running_mean", "layers.3.weight", "layers.7.bias",
              "layers.8.0.layers.0.weight", "layers.12.3.layers.7.weight",
              "layers.13.0.layers.4.num_batches_tracked",
              "layers.15.running_var", "classifier.1.bias"]:
        assert k in sd, k
    assert tuple(sd["layers.0.weight"].shape) == (32, 3, 3, 3)
    assert tuple(sd["layers.9.0.layers.3.weight"].shape) == (72, 1, 5, 5)
    assert tuple(sd["layers.14.weight"].shape) == (1280, 320, 1, 1)
    assert tuple(sd["classifier.1.weight"].shape) == (1000, 1280)
    assert net1000.layers[1].momentum == pytest.approx(1 - 0.9997)


def test_conv_census(net1000):
    convs = [m for m in net1000.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 52
    assert all(isinstance(c, AmdConv2d) and c.bias is None for c in convs)
    dw = [c for c in convs if c.groups == c.in_channels and c.groups > 1]
    assert all(c.out_channels == c.in_channels and c.in_channels % 8 == 0
               for c in dw)
    dw5 = [c for c in dw if c.kernel_size == (5, 5)]
    dw3 = [c for c in dw if c.kernel_size == (3, 3)]
    assert (len(dw5), len(dw3), len(dw)) == (10, 7, 17)
    assert all(c.padding == (c.kernel_size[0] // 2,) * 2 for c in dw)


def test_registry_and_parser():
    assert {"mnasnet1_0", "mnasnet0_5"} <= set(model_names())
    assert not {"mnasnet0_75", "mnasnet1_3"} & set(model_names())
    args = base_parser("t").parse_args(["-a", "mnasnet1_0"])
    assert args.arch == "mnasnet1_0"


def test_forward_backward_cpu():
    torch.manual_seed(0)
    m = build_model("mnasnet1_0", num_classes=10).train()
    y = m(torch.randn(2, 3, 64, 64))
    assert y.shape == (2, 10)
    y.sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv5x5_cpu_is_conv2d(stride):
    torch.manual_seed(stride)
    x = torch.randn(2, 16, 9, 7)
    w = torch.randn(16, 1, 5, 5)
    ref = F.conv2d(x, w, None, stride, 2, 1, 16)
    out = dwconv5x5(x, w, stride)
    assert out.shape == ref.shape and torch.equal(out, ref)
