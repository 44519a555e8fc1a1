"""Architecture registry: the one table behind ``-a/--arch``,
``model_names()`` and ``build_model()``."""

from __future__ import annotations

from typing import Callable, Dict, List

import torch.nn as nn

from .mobilenet import mobilenet_v2
from .resnet import (resnet18, resnet34, resnet50, resnet101, resnet152,
                     resnext50_32x4d, wide_resnet50_2)

_REGISTRY: Dict[str, Callable[..., nn.Module]] = {
    "resnet18": resnet18,
    "resnet34": resnet34,
    "resnet50": resnet50,
    "resnet101": resnet101,
    "resnet152": resnet152,
    "resnext50_32x4d": resnext50_32x4d,
    "wide_resnet50_2": wide_resnet50_2,
    "mobilenet_v2": mobilenet_v2,
}


def model_names() -> List[str]:
    """Sorted architecture names, for the ``-a/--arch`` choices list
    (reference distributed.py:21-23)."""
    return sorted(_REGISTRY)


def build_model(arch: str, num_classes: int = 1000, **kw) -> nn.Module:
    """``torchvision.models.__dict__[arch]()`` equivalent (distributed.py:134-139)."""
    if arch not in _REGISTRY:
        raise ValueError(f"unknown arch '{arch}'; choices: {model_names()}")
    return _REGISTRY[arch](num_classes=num_classes, **kw)
