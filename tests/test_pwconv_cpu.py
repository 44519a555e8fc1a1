"""Routing of the thin pointwise (1x1) conv kernel, checked without a GPU:
the pure-Python predicate ``pw_thin_ok`` over mobilenet_v2's pointwise
layers, the CPU behaviour of the layers it takes, and the unchanged module
tree."""

import torch
import torch.nn as nn
import torch.nn.functional as F

from amdtrain.models import build_model
from amdtrain.ops.conv import AmdConv2d, pw_thin_ok

THIN = sorted([(32, 16), (16, 96), (96, 24), (24, 144), (24, 144),
               (144, 24), (144, 32)])


def _pointwise_pairs(model):
    return [(m.in_channels, m.out_channels) for m in model.modules()
            if isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1)]


def test_mobilenet_pointwise_table():
    pairs = _pointwise_pairs(build_model("mobilenet_v2"))
    assert len(pairs) == 34
    gemm = [p for p in pairs if p[0] % 32 == 0 and p[1] % 32 == 0]
    thin = [p for p in pairs if pw_thin_ok(*p)]
    assert len(gemm) == 27 and len(thin) == 7
    assert not set(gemm) & set(thin)
    assert sorted(thin) == THIN
    assert sorted(gemm + thin) == sorted(pairs)     # none goes elsewhere


def test_pw_thin_ok_outside_the_contract():
    assert not pw_thin_ok(12, 24)       # K % 8
    assert not pw_thin_ok(24, 20)       # N % 8
    assert not pw_thin_ok(160, 160)     # over the LDS bound
    assert not pw_thin_ok(32, 64)       # the MFMA GEMM's
    assert not pw_thin_ok(0, 8) and not pw_thin_ok(8, 0)
    # both orientations are the same question
    for k, n in [(32, 16), (8, 160), (40, 56), (264, 8), (8, 264)]:
        assert pw_thin_ok(k, n) == pw_thin_ok(n, k)
    assert pw_thin_ok(8, 8) and pw_thin_ok(40, 56) and pw_thin_ok(8, 160)
    assert not pw_thin_ok(264, 8)       # ceil32(264) = 288: 9 blocks


def test_amdconv2d_cpu_equals_conv2d(monkeypatch):
    g = torch.Generator().manual_seed(24144)
    conv = AmdConv2d(24, 144, 1, bias=False)
    x = torch.randn(2, 24, 5, 7, generator=g)
    for flag in ("1", "0"):
        monkeypatch.setenv("AMDTRAIN_PWCONV", flag)
        assert torch.equal(conv(x), F.conv2d(x, conv.weight))


def test_library_conv_on_cpu(monkeypatch):
    from amdtrain.models.mobilenet import LibraryConv2d
    g = torch.Generator().manual_seed(3216)
    conv = LibraryConv2d(32, 16, 1, bias=False)
    x = torch.randn(2, 32, 5, 7, generator=g)
    for flag in ("1", "0"):
        monkeypatch.setenv("AMDTRAIN_PWCONV", flag)
        assert torch.equal(conv(x), F.conv2d(x, conv.weight))


def test_state_dict_keys_unchanged():
    """The keys are torchvision's: 52 conv, 52 x 5 BN and 2 classifier
    entries, and features.1.conv.1 is still the 32 -> 16 LibraryConv2d."""
    from amdtrain.models.mobilenet import LibraryConv2d
    m = build_model("mobilenet_v2")
    keys = list(m.state_dict().keys())
    assert len(keys) == 52 + 52 * 5 + 2
    assert keys[0] == "features.0.0.weight"
    assert "features.1.conv.1.weight" in keys
    assert "features.2.conv.0.0.weight" in keys
    assert "features.18.0.weight" in keys
    assert keys[-2:] == ["classifier.1.weight", "classifier.1.bias"]
    pin = m.features[1].conv[1]
    assert isinstance(pin, LibraryConv2d)
    assert (pin.in_channels, pin.out_channels) == (32, 16)
    assert sum(isinstance(x, LibraryConv2d) for x in m.modules()) == 1
