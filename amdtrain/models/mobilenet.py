"""Native MobileNetV2 for ImageNet (Sandler et al. 2018, "MobileNetV2:
Inverted Residuals and Linear Bottlenecks").

Written from the paper; torchvision is not a dependency.  The module tree
is laid out so that the ``state_dict`` keys are torchvision's
(``features.N.conv...``, ``classifier.1``), so its checkpoints load
unchanged.

Every conv is an ``AmdConv2d``: the 17 depthwise 3x3 layers run on the
stencil kernels of ``ops/csrc/dwconv.hip``; the pointwise layers and the stem
take whatever path ``AmdConv2d`` has for their shape (docs/KERNELS.md lists
them).  Every BN is a ``FusedBatchNorm2d`` that runs through
``ops.fused.batch_norm``: the 35 BN -> ReLU6 pairs with ``relu6=True``, one
apply pass with the clamp in its epilogue, and the 17 linear-bottleneck BNs
without an activation, the 10 of them that close an identity shortcut with
the shortcut as the BN's ``addend``, so that ``x + out`` is no pass of its
own in either direction.  The widths that are no power of two (42 of the 52
BNs) run on the any-C kernels of ``ops/csrc/batchnorm_anyc.h``.  A width
those kernels do not take (fp32 without autocast: C = 1280 is 320 packs)
keeps BN followed by ``F.relu6``.
"""

from __future__ import annotations

from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import fused as OF
from ..ops.conv import AmdConv2d, _pwconv_enabled, pw_thin_ok
from ..ops.linear import AmdLinear
from .resnet import FusedBatchNorm2d

# (expansion t, output channels c, repeats n, stride s), paper table 2
_SETTINGS = [
    (1, 16, 1, 1),
    (6, 24, 2, 2),
    (6, 32, 3, 2),
    (6, 64, 4, 2),
    (6, 96, 3, 1),
    (6, 160, 3, 2),
    (6, 320, 1, 1),
]


class LibraryConv2d(AmdConv2d):
    """An ``AmdConv2d`` that keeps off the MFMA GEMM: it runs on the thin
    pointwise kernel when that is enabled and takes the layer, and on the
    library (``nn.Conv2d``) path otherwise."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if (_pwconv_enabled() and self.kernel_size == (1, 1)
                and self.stride == (1, 1)
                and pw_thin_ok(self.in_channels, self.out_channels)):
            return AmdConv2d.forward(self, x)
        return nn.Conv2d.forward(self, x)


def _pointwise(inp: int, oup: int) -> AmdConv2d:
    """1x1 conv.  ``AmdConv2d`` sends in % 32 == 0, out % 32 == 0 to the
    MFMA GEMM and the other widths of this model (``pw_thin_ok``) to the thin
    pointwise kernel of ``ops/csrc/pwconv.hip``.  With that kernel switched
    off (AMDTRAIN_PWCONV=0) in % 32 == 0, out % 16 == 0 goes to the GEMM,
    whose input gradient then needs out % 32 == 0 as its K and raises
    otherwise; the one such layer here (32 -> 16, features.1) is a
    ``LibraryConv2d``, which takes the library path in that case.

    The first two terms of the condition repeat ``ch_ok`` of
    ``AmdConv2d.forward`` (ops/conv.py); if that guard changes, change this
    with it."""
    if inp % 32 == 0 and oup % 16 == 0 and oup % 32 != 0:
        return LibraryConv2d(inp, oup, 1, bias=False)
    return AmdConv2d(inp, oup, 1, bias=False)


class ConvBNReLU6(nn.Sequential):
    """conv -> BN -> ReLU6 as ``.0`` / ``.1`` / ``.2`` (torchvision keys)."""

    def __init__(self, inp: int, oup: int, kernel_size: int = 3,
                 stride: int = 1, groups: int = 1):
        super().__init__(
            AmdConv2d(inp, oup, kernel_size, stride=stride,
                      padding=(kernel_size - 1) // 2, groups=groups,
                      bias=False),
            FusedBatchNorm2d(oup),
            nn.ReLU6(inplace=True),  # kept for module-tree parity
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self[0](x)
        if OF.bn_relu6_fusable(y):
            return OF.batch_norm(y, self[1], relu6=True)
        # no ReLU6 kernel for this width and dtype (fp32 C = 1280): the
        # two ops, as before the fusion
        return F.relu6(OF.batch_norm(y, self[1], relu=False))


class InvertedResidual(nn.Module):
    """1x1 expand (absent when t == 1) -> 3x3 depthwise -> linear 1x1
    project; identity shortcut when the block keeps shape."""

    def __init__(self, inp: int, oup: int, stride: int, expand_ratio: int):
        super().__init__()
        assert stride in (1, 2)
        hidden = inp * expand_ratio
        self.use_res_connect = stride == 1 and inp == oup
        layers: List[nn.Module] = []
        if expand_ratio != 1:
            layers.append(ConvBNReLU6(inp, hidden, kernel_size=1))
        layers += [
            ConvBNReLU6(hidden, hidden, stride=stride, groups=hidden),
            _pointwise(hidden, oup),
            FusedBatchNorm2d(oup),
        ]
        self.conv = nn.Sequential(*layers)
        self._n_act = len(layers) - 2   # ConvBNReLU6 stages before project

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = x
        for i in range(self._n_act):   # expand (if any) and depthwise
            out = self.conv[i](out)
        # the identity shortcut rides in the BN apply as its addend
        return OF.batch_norm(self.conv[self._n_act](out),
                             self.conv[self._n_act + 1], relu=False,
                             addend=x if self.use_res_connect else None)


class MobileNetV2(nn.Module):
    def __init__(self, num_classes: int = 1000, dropout: float = 0.2):
        super().__init__()
        inp, last = 32, 1280
        features: List[nn.Module] = [ConvBNReLU6(3, inp, stride=2)]
        for t, c, n, s in _SETTINGS:
            for i in range(n):
                features.append(
                    InvertedResidual(inp, c, s if i == 0 else 1, t))
                inp = c
        features.append(ConvBNReLU6(inp, last, kernel_size=1))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(
            nn.Dropout(p=dropout),
            AmdLinear(last, num_classes),
        )

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        x = OF.global_avg_pool(x)
        x = torch.flatten(x, 1)
        return self.classifier(x)


def mobilenet_v2(num_classes: int = 1000, **kw) -> MobileNetV2:
    return MobileNetV2(num_classes=num_classes, **kw)
