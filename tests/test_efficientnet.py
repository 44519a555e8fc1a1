"""EfficientNet-B0: torchvision-compatible layout, registry entry, and the CPU
paths of BN -> SiLU and of the SiLU / sigmoid squeeze-excite."""
import pytest
import torch
import torch.nn.functional as F

from amdtrain.config import base_parser
from amdtrain.models import EfficientNet, build_model, model_names
from amdtrain.models.resnet import FusedBatchNorm2d
from amdtrain.ops import fused, squeeze_excite


def test_layout_and_registry():
    m = build_model("efficientnet_b0")
    assert isinstance(m, EfficientNet)
    assert sum(p.numel() for p in m.parameters()) == 5_288_548
    sd = m.state_dict()
    for k, shape in [
        ("features.0.0.weight", (32, 3, 3, 3)),
        ("features.1.0.block.0.0.weight", (32, 1, 3, 3)),   # no expand conv
        ("features.1.0.block.1.fc1.weight", (8, 32, 1, 1)),
        ("features.2.0.block.0.0.weight", (96, 16, 1, 1)),
        ("features.2.0.block.3.1.running_var", (24,)),
        ("features.8.1.weight", (1280,)),
        ("classifier.1.weight", (1000, 1280)),
    ]:
        assert tuple(sd[k].shape) == shape, k
    assert "efficientnet_b0" in model_names()
    assert base_parser("t").parse_args(["-a", "efficientnet_b0"]).arch \
        == "efficientnet_b0"


def test_forward_cpu():
    torch.manual_seed(0)
    y = build_model("efficientnet_b0").train()(torch.randn(2, 3, 64, 64))
    assert y.shape == (2, 1000) and torch.isfinite(y).all()


def test_batch_norm_silu_cpu_is_the_composition():
    torch.manual_seed(1)
    bn = FusedBatchNorm2d(24).train()
    x = torch.randn(2, 24, 5, 5)
    ref = F.silu(F.batch_norm(x, None, None, bn.weight, bn.bias, True))
    assert torch.equal(fused.batch_norm(x, bn, silu=True), ref)
    for kw in (dict(relu=True), dict(relu6=True), dict(addend=x)):
        with pytest.raises(ValueError):
            fused.batch_norm(x, bn, silu=True, **kw)


def test_squeeze_excite_silu_sigmoid_cpu_is_the_composition():
    g = torch.Generator().manual_seed(2)
    x = 3 * torch.randn(2, 16, 5, 3, generator=g)
    w1, b1 = torch.randn(4, 16, generator=g), torch.randn(4, generator=g)
    w2, b2 = torch.randn(16, 4, generator=g), torch.randn(16, generator=g)
    s = torch.sigmoid(F.linear(F.silu(F.linear(x.mean((2, 3)), w1, b1)),
                               w2, b2))
    y = squeeze_excite(x, w1, b1, w2, b2, hidden_act="silu", gate="sigmoid")
    assert torch.equal(y, x * s[:, :, None, None])
