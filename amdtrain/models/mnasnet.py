"""Native MNASNet for ImageNet (Tan et al. 2019, "MnasNet: Platform-Aware
Neural Architecture Search for Mobile", the MnasNet-A1-like B1 network
without squeeze-excite).

Written from the paper and the published layer table; torchvision is not a
dependency.  The module tree is laid out so that the ``state_dict`` keys are
torchvision's (``layers.0`` ... ``layers.16``, blocks as
``layers.N.M.layers.0..7``, ``classifier.1``), so its checkpoints load
unchanged.

Every conv is an ``AmdConv2d``.  At depth multiplier 1.0: the 10 depthwise
5x5 layers run on the halo-tile kernels of ``ops/csrc/dwconv5x5.hip``, the 7
depthwise 3x3 layers on the stencils of ``ops/csrc/dwconv.hip``, the 34 1x1
layers on the pointwise kernels (all widths are multiples of 8; see
``mobilenet._pointwise``) and the stem on the generic path.  Every BN runs
through ``ops.fused.batch_norm``: BN+ReLU after the expansion and the
depthwise conv, and a linear BN at the end of a block with the identity
shortcut as its ``addend``.
"""

from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from ..ops import fused as OF
from ..ops.conv import AmdConv2d
from ..ops.linear import AmdLinear
from .mobilenet import _make_divisible, _pointwise
from .resnet import FusedBatchNorm2d

# torchvision's momentum is 1 - TensorFlow's decay of 0.9997
_BN_MOMENTUM = 1 - 0.9997

# (output depth index, kernel, stride, expansion, repeats), paper figure 7
_STACKS = [
    (2, 3, 2, 3, 3),
    (3, 5, 2, 3, 3),
    (4, 5, 2, 6, 3),
    (5, 3, 1, 6, 2),
    (6, 5, 2, 6, 4),
    (7, 3, 1, 6, 1),
]
_DEPTHS = [32, 16, 24, 40, 80, 96, 192, 320]


def _bn(c: int) -> FusedBatchNorm2d:
    return FusedBatchNorm2d(c, momentum=_BN_MOMENTUM)


def _depthwise(c: int, kernel: int, stride: int) -> AmdConv2d:
    return AmdConv2d(c, c, kernel, padding=kernel // 2, stride=stride,
                     groups=c, bias=False)


class _InvertedResidual(nn.Module):
    """1x1 expand -> k x k depthwise -> linear 1x1 project as
    ``layers.0..7`` (conv, BN, ReLU, conv, BN, ReLU, conv, BN); identity
    shortcut when the block keeps shape."""

    def __init__(self, inp: int, oup: int, kernel: int, stride: int,
                 expansion: int):
        super().__init__()
        assert stride in (1, 2) and kernel in (3, 5)
        mid = inp * expansion
        self.apply_residual = inp == oup and stride == 1
        self.layers = nn.Sequential(
            _pointwise(inp, mid), _bn(mid), nn.ReLU(inplace=True),
            _depthwise(mid, kernel, stride), _bn(mid), nn.ReLU(inplace=True),
            _pointwise(mid, oup), _bn(oup))  # ReLUs: module-tree parity

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        L = self.layers
        out = OF.batch_norm(L[0](x), L[1], relu=True)
        out = OF.batch_norm(L[3](out), L[4], relu=True)
        # the identity shortcut rides in the BN apply as its addend
        return OF.batch_norm(L[6](out), L[7], relu=False,
                             addend=x if self.apply_residual else None)


def _stack(inp: int, oup: int, kernel: int, stride: int, expansion: int,
           repeats: int) -> nn.Sequential:
    blocks = [_InvertedResidual(inp, oup, kernel, stride, expansion)]
    blocks += [_InvertedResidual(oup, oup, kernel, 1, expansion)
               for _ in range(repeats - 1)]
    return nn.Sequential(*blocks)


class MNASNet(nn.Module):
    """``alpha`` scales every depth, rounded to a multiple of 8
    (``_make_divisible``); the 1280-wide head stays."""

    def __init__(self, alpha: float, num_classes: int = 1000,
                 dropout: float = 0.2):
        super().__init__()
        assert alpha > 0.0
        d = [_make_divisible(c * alpha, 8) for c in _DEPTHS]
        layers: List[nn.Module] = [
            AmdConv2d(3, d[0], 3, padding=1, stride=2, bias=False),
            _bn(d[0]), nn.ReLU(inplace=True),
            _depthwise(d[0], 3, 1), _bn(d[0]), nn.ReLU(inplace=True),
            _pointwise(d[0], d[1]), _bn(d[1]),
        ]
        inp = d[1]
        for i, kernel, stride, expansion, repeats in _STACKS:
            layers.append(_stack(inp, d[i], kernel, stride, expansion,
                                 repeats))
            inp = d[i]
        layers += [_pointwise(inp, 1280), _bn(1280), nn.ReLU(inplace=True)]
        self.layers = nn.Sequential(*layers)
        self.classifier = nn.Sequential(
            nn.Dropout(p=dropout),
            AmdLinear(1280, num_classes),
        )

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight, mode="fan_out",
                                         nonlinearity="sigmoid")
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        L = self.layers
        x = OF.batch_norm(L[0](x), L[1], relu=True)
        x = OF.batch_norm(L[3](x), L[4], relu=True)
        x = OF.batch_norm(L[6](x), L[7], relu=False)
        for i in range(8, 14):
            x = L[i](x)
        x = OF.batch_norm(L[14](x), L[15], relu=True)
        x = OF.global_avg_pool(x)
        x = torch.flatten(x, 1)
        return self.classifier(x)


def mnasnet1_0(num_classes: int = 1000, **kw) -> MNASNet:
    return MNASNet(1.0, num_classes=num_classes, **kw)


def mnasnet0_5(num_classes: int = 1000, **kw) -> MNASNet:
    return MNASNet(0.5, num_classes=num_classes, **kw)


def mnasnet0_75(num_classes: int = 1000, **kw) -> MNASNet:
    """Depths 24, 16, 24, 32, 64, 72, 144, 240; the 24-wide stem runs on the
    direct RGB stem kernels (``ops/csrc/stem3x3.hip``).  Exported from
    ``amdtrain.models`` but not yet a registry name: ``tests/test_mnasnet.py``
    pins 0.75 and 1.3 as absent from ``model_names()``."""
    return MNASNet(0.75, num_classes=num_classes, **kw)


def mnasnet1_3(num_classes: int = 1000, **kw) -> MNASNet:
    """Depths 40, 24, 32, 56, 104, 128, 248, 416; 40-wide stem as above."""
    return MNASNet(1.3, num_classes=num_classes, **kw)
