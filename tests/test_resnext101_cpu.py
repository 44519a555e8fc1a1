"""resnext101_32x8d / resnext101_64x4d in the registry: names, parameter
counts (torchvision's) and the grouped-conv shapes the per-group kernel
serves."""
import pytest
import torch

from amdtrain.models import build_model, model_names
from amdtrain.ops.conv import gconv_ok


@pytest.mark.parametrize("arch,params", [("resnext101_32x8d", 88_791_336),
                                         ("resnext101_64x4d", 83_455_272)])
def test_registered_with_torchvision_param_count(arch, params):
    assert arch in model_names()
    model = build_model(arch)
    assert sum(p.numel() for p in model.parameters()) == params


def test_64x4d_grouped_convs_fit_the_per_group_kernel():
    convs = [m for m in build_model("resnext101_64x4d").modules()
             if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    assert len(convs) == 33
    assert {m.in_channels // m.groups for m in convs} == {4, 8, 16, 32}
    assert all(gconv_ok(m.in_channels, m.out_channels, m.groups)
               for m in convs)
