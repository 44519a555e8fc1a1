"""MobileNetV2: torchvision-compatible layout, registry entry, CPU paths."""
import pytest
import torch
import torch.nn.functional as F

from amdtrain.config import base_parser
from amdtrain.models import MobileNetV2, build_model, model_names
from amdtrain.ops.conv import AmdConv2d, dwconv3x3


@pytest.fixture(scope="module")
def net1000():
    return build_model("mobilenet_v2")


def test_param_count(net1000):
    assert isinstance(net1000, MobileNetV2)
    assert sum(p.numel() for p in net1000.parameters()) == 3_504_872


def test_state_dict_layout(net1000):
    sd = net1000.state_dict()
    assert len(sd) == 314
    for k in ["features.0.0.weight",
              "features.1.conv.0.0.weight",
              "features.1.conv.1.weight",
              "features.1.conv.2.running_var",
              "features.2.conv.1.0.weight",
              "features.2.conv.2.weight",
              "features.2.conv.3.bias",
              "features.17.conv.3.weight",
              "features.18.1.num_batches_tracked",
              "classifier.1.weight"]:
        assert k in sd, k
    assert tuple(sd["features.2.conv.1.0.weight"].shape) == (96, 1, 3, 3)
    assert tuple(sd["features.0.0.weight"].shape) == (32, 3, 3, 3)
    assert tuple(sd["features.18.0.weight"].shape) == (1280, 320, 1, 1)
    assert tuple(sd["classifier.1.weight"].shape) == (1000, 1280)


def test_conv_layer_types(net1000):
    convs = [m for m in net1000.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 52
    assert all(isinstance(c, AmdConv2d) for c in convs)
    dw = [c for c in convs if c.groups == c.in_channels and c.groups > 1]
    assert len(dw) == 17
    for c in dw:
        assert c.kernel_size == (3, 3) and c.padding == (1, 1)
        assert c.out_channels == c.in_channels and c.in_channels % 8 == 0
        assert c.bias is None


def test_forward_backward_cpu():
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10)
    m.train()
    x = torch.randn(2, 3, 64, 64)
    y = m(x)
    assert y.shape == (2, 10)
    y.sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad).all(), name


def test_eval_keeps_running_stats():
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10)
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()
              if "running_" in k or "num_batches" in k}
    assert len(before) == 52 * 3
    with torch.no_grad():
        m(torch.randn(2, 3, 64, 64))
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_registry_and_parser():
    assert "mobilenet_v2" in model_names()
    assert "resnet50" in model_names()
    args = base_parser("t").parse_args(["-a", "mobilenet_v2"])
    assert args.arch == "mobilenet_v2"


@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv3x3_cpu_is_conv2d(stride):
    torch.manual_seed(stride)
    x = torch.randn(2, 16, 9, 7)
    w = torch.randn(16, 1, 3, 3)
    ref = F.conv2d(x, w, None, stride, 1, 1, 16)
    out = dwconv3x3(x, w, stride)
    assert out.shape == ref.shape
    assert torch.equal(out, ref)
