"""Native MobileNetV3 for ImageNet (Howard et al. 2019, "Searching for
MobileNetV3", tables 1 and 2).

Written from the paper; torchvision is not a dependency.  The module tree
is laid out so that the ``state_dict`` keys are torchvision's
(``features.0.0/1``, ``features.N.block.M.0/1`` with ``fc1`` / ``fc2`` inside
the squeeze-excite member, the last conv, ``classifier.0`` / ``classifier.3``),
so its checkpoints load unchanged.  A block whose expansion equals its input
width has no expand conv and its members shift down by one, as there.

Every conv is an ``AmdConv2d`` and every width is a multiple of 8: the
depthwise 3x3 and 5x5 layers run on the stencil and halo-tile kernels, the
1x1 layers on the pointwise kernels (``mobilenet._pointwise``), the 3 -> 16
stem on the generic path.  Activation wiring:

  * BN -> ReLU is ``ops.fused.batch_norm(relu=True)``;
  * BN -> hardswish directly before a squeeze-excite block is a linear BN
    followed by ``SqueezeExcite(pre_act="hardswish")``: the activation
    happens inside the SE kernels and is no pass of its own;
  * every other BN -> hardswish is a linear BN followed by ``ops.hardswish``;
  * project BNs are linear, with the identity shortcut as their ``addend``.
"""

from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from ..ops import fused as OF
from ..ops.conv import AmdConv2d
from ..ops.linear import AmdLinear
from ..ops.se import SqueezeExcite, hardswish
from .mobilenet import _make_divisible, _pointwise
from .resnet import FusedBatchNorm2d

# (kernel, expanded, out, squeeze-excite, activation, stride)
_LARGE = [
    (3, 16, 16, False, "RE", 1),
    (3, 64, 24, False, "RE", 2),
    (3, 72, 24, False, "RE", 1),
    (5, 72, 40, True, "RE", 2),
    (5, 120, 40, True, "RE", 1),
    (5, 120, 40, True, "RE", 1),
    (3, 240, 80, False, "HS", 2),
    (3, 200, 80, False, "HS", 1),
    (3, 184, 80, False, "HS", 1),
    (3, 184, 80, False, "HS", 1),
    (3, 480, 112, True, "HS", 1),
    (3, 672, 112, True, "HS", 1),
    (5, 672, 160, True, "HS", 2),
    (5, 960, 160, True, "HS", 1),
    (5, 960, 160, True, "HS", 1),
]
_SMALL = [
    (3, 16, 16, True, "RE", 2),
    (3, 72, 24, False, "RE", 2),
    (3, 88, 24, False, "RE", 1),
    (5, 96, 40, True, "HS", 2),
    (5, 240, 40, True, "HS", 1),
    (5, 240, 40, True, "HS", 1),
    (5, 120, 48, True, "HS", 1),
    (5, 144, 48, True, "HS", 1),
    (5, 288, 96, True, "HS", 2),
    (5, 576, 96, True, "HS", 1),
    (5, 576, 96, True, "HS", 1),
]


class _ConvBNAct(nn.Sequential):
    """conv -> BN (-> activation) as ``.0`` / ``.1`` (/ ``.2``).  ``act`` is
    "RE", "HS" or None; ``fuse_act=False`` leaves a hardswish to the consumer
    (the squeeze-excite block that follows)."""

    def __init__(self, conv: AmdConv2d, act: Optional[str]):
        layers: List[nn.Module] = [
            conv, FusedBatchNorm2d(conv.out_channels, eps=1e-3, momentum=0.01)]
        if act is not None:  # kept for module-tree parity
            layers.append(nn.ReLU(inplace=True) if act == "RE"
                          else nn.Hardswish())
        super().__init__(*layers)
        self.act = act

    def forward(self, x: torch.Tensor, addend: Optional[torch.Tensor] = None,
                fuse_act: bool = True) -> torch.Tensor:
        y = OF.batch_norm(self[0](x), self[1], relu=self.act == "RE",
                          addend=addend)
        if self.act == "HS" and fuse_act:
            y = hardswish(y)
        return y


class InvertedResidualV3(nn.Module):
    """1x1 expand (absent when expanded == inp) -> k x k depthwise ->
    squeeze-excite (optional) -> linear 1x1 project, as ``block.0..``;
    identity shortcut when the block keeps shape."""

    def __init__(self, inp: int, kernel: int, exp: int, oup: int, se: bool,
                 act: str, stride: int):
        super().__init__()
        assert stride in (1, 2) and kernel in (3, 5) and act in ("RE", "HS")
        self.use_res_connect = stride == 1 and inp == oup
        layers: List[nn.Module] = []
        if exp != inp:
            layers.append(_ConvBNAct(_pointwise(inp, exp), act))
        layers.append(_ConvBNAct(
            AmdConv2d(exp, exp, kernel, stride=stride, padding=kernel // 2,
                      groups=exp, bias=False), act))
        if se:
            layers.append(SqueezeExcite(
                exp, _make_divisible(exp // 4, 8),
                pre_act="hardswish" if act == "HS" else "none"))
        layers.append(_ConvBNAct(_pointwise(exp, oup), None))
        self.block = nn.Sequential(*layers)
        self._expand = exp != inp
        self._se = se

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B = self.block
        out, i = x, 0
        if self._expand:
            out, i = B[0](out), 1
        if self._se:
            # the hardswish of an HS block is applied inside the SE kernels
            out = B[i + 1](B[i](out, fuse_act=False))
            i += 2
        else:
            out = B[i](out)
            i += 1
        # the identity shortcut rides in the BN apply as its addend
        return B[i](out, addend=x if self.use_res_connect else None)


class MobileNetV3(nn.Module):
    def __init__(self, settings, last_channel: int, num_classes: int = 1000,
                 dropout: float = 0.2):
        super().__init__()
        features: List[nn.Module] = [_ConvBNAct(
            AmdConv2d(3, 16, 3, stride=2, padding=1, bias=False), "HS")]
        inp = 16
        for kernel, exp, oup, se, act, stride in settings:
            features.append(InvertedResidualV3(inp, kernel, exp, oup, se, act,
                                               stride))
            inp = oup
        features.append(_ConvBNAct(_pointwise(inp, 6 * inp), "HS"))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(
            AmdLinear(6 * inp, last_channel),
            nn.Hardswish(),  # module-tree parity; forward calls ops.hardswish
            nn.Dropout(p=dropout),
            AmdLinear(last_channel, num_classes),
        )

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        x = torch.flatten(OF.global_avg_pool(x), 1)
        C = self.classifier
        x = hardswish(C[0](x))
        return C[3](C[2](x))


def mobilenet_v3_large(num_classes: int = 1000, **kw) -> MobileNetV3:
    return MobileNetV3(_LARGE, 1280, num_classes=num_classes, **kw)


def mobilenet_v3_small(num_classes: int = 1000, **kw) -> MobileNetV3:
    return MobileNetV3(_SMALL, 1024, num_classes=num_classes, **kw)
