"""Native EfficientNet-B0 for ImageNet (Tan & Le 2019, "EfficientNet:
Rethinking Model Scaling for Convolutional Neural Networks", table 1).

Written from the paper; torchvision is not a dependency.  The module tree
is laid out so that the ``state_dict`` keys are torchvision's
(``features.0.0/1``, ``features.S.R.block.M.0/1`` for repeat R of stage S
with ``fc1`` / ``fc2`` inside the squeeze-excite member, ``features.8.0/1``,
``classifier.1``), so its checkpoints load unchanged.  Stage 1 expands by 1
and has no expand conv: its members shift down by one, as there.

Every conv is an ``AmdConv2d`` and every width is a multiple of 8: the
depthwise 3x3 and 5x5 layers run on the stencil and halo-tile kernels, the
1x1 layers on the pointwise kernels (``mobilenet._pointwise``), the 3 -> 32
stem on the generic path.  Activation wiring:

  * stem, expand, depthwise and head BN -> SiLU are
    ``ops.fused.batch_norm(silu=True)``: one apply pass that writes the
    activated tensor, a backward that recomputes the slope;
  * the squeeze-excite block (SiLU inside, sigmoid gate) runs on that
    activated depthwise output with ``pre_act="none"``, so its backward
    apply does not read its input at all.  MobileNetV3 does it the other way
    round (linear BN, hardswish inside the SE kernels);
  * project BNs are linear, with the identity shortcut as their ``addend``.

Stochastic depth (row mode, block i of 16 drops with ``p * i / 16``) is
plain torch ops on an [N, 1, 1, 1] mask; where it is active (training,
``p_i > 0``) the shortcut is an eager add and not the BN's addend.
"""

from __future__ import annotations

import math
from typing import List

import torch
import torch.nn as nn

from ..ops import fused as OF
from ..ops.conv import AmdConv2d
from ..ops.linear import AmdLinear
from ..ops.se import SqueezeExcite
from .mobilenet import _pointwise
from .resnet import FusedBatchNorm2d

# (expand, kernel, stride, in, out, repeats), paper table 1
_B0 = [
    (1, 3, 1, 32, 16, 1),
    (6, 3, 2, 16, 24, 2),
    (6, 5, 2, 24, 40, 2),
    (6, 3, 2, 40, 80, 3),
    (6, 5, 1, 80, 112, 3),
    (6, 5, 2, 112, 192, 4),
    (6, 3, 1, 192, 320, 1),
]


class _ConvBN(nn.Sequential):
    """conv -> BN (-> SiLU) as ``.0`` / ``.1`` (/ ``.2``)."""

    def __init__(self, conv: AmdConv2d, silu: bool):
        layers: List[nn.Module] = [
            conv, FusedBatchNorm2d(conv.out_channels, eps=1e-5, momentum=0.1)]
        if silu:  # kept for module-tree parity
            layers.append(nn.SiLU(inplace=True))
        super().__init__(*layers)
        self.silu = silu

    def forward(self, x: torch.Tensor, addend=None) -> torch.Tensor:
        return OF.batch_norm(self[0](x), self[1], silu=self.silu,
                             addend=addend)


class MBConv(nn.Module):
    """1x1 expand (absent when expand == 1) -> k x k depthwise ->
    squeeze-excite -> linear 1x1 project, as ``block.0..``; identity
    shortcut, under stochastic depth, when the block keeps shape."""

    def __init__(self, inp: int, oup: int, kernel: int, stride: int,
                 expand: int, sd_prob: float):
        super().__init__()
        assert stride in (1, 2) and kernel in (3, 5)
        self.use_res_connect = stride == 1 and inp == oup
        self.sd_prob = sd_prob
        exp = inp * expand
        layers: List[nn.Module] = []
        if exp != inp:
            layers.append(_ConvBN(_pointwise(inp, exp), True))
        layers += [
            _ConvBN(AmdConv2d(exp, exp, kernel, stride=stride,
                              padding=kernel // 2, groups=exp, bias=False),
                    True),
            SqueezeExcite(exp, max(1, inp // 4), pre_act="none",
                          hidden_act="silu", gate="sigmoid"),
            _ConvBN(_pointwise(exp, oup), False),
        ]
        self.block = nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = x
        for i in range(len(self.block) - 1):   # expand (if any), dw, SE
            out = self.block[i](out)
        if not self.use_res_connect:
            return self.block[-1](out)
        if not (self.training and self.sd_prob > 0.0):
            # the identity shortcut rides in the BN apply as its addend
            return self.block[-1](out, addend=x)
        keep = 1.0 - self.sd_prob
        mask = torch.empty(x.shape[0], 1, 1, 1, dtype=x.dtype,
                           device=x.device).bernoulli_(keep).div_(keep)
        return self.block[-1](out) * mask + x


class EfficientNet(nn.Module):
    def __init__(self, settings, num_classes: int = 1000,
                 dropout: float = 0.2, stochastic_depth_prob: float = 0.2):
        super().__init__()
        features: List[nn.Module] = [_ConvBN(
            AmdConv2d(3, settings[0][3], 3, stride=2, padding=1, bias=False),
            True)]
        total = sum(s[5] for s in settings)
        done = 0
        for expand, kernel, stride, inp, oup, repeats in settings:
            stage: List[nn.Module] = []
            for r in range(repeats):
                stage.append(MBConv(
                    inp if r == 0 else oup, oup, kernel,
                    stride if r == 0 else 1, expand,
                    stochastic_depth_prob * done / total))
                done += 1
            features.append(nn.Sequential(*stage))
        last = settings[-1][4]
        features.append(_ConvBN(_pointwise(last, 4 * last), True))
        self.features = nn.Sequential(*features)
        self.classifier = nn.Sequential(
            nn.Dropout(p=dropout),
            AmdLinear(4 * last, num_classes),
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
                bound = 1.0 / math.sqrt(m.out_features)
                nn.init.uniform_(m.weight, -bound, bound)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.features(x)
        x = torch.flatten(OF.global_avg_pool(x), 1)
        return self.classifier(x)


def efficientnet_b0(num_classes: int = 1000, **kw) -> EfficientNet:
    return EfficientNet(_B0, num_classes=num_classes, **kw)
