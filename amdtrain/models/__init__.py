from .resnet import (
    ResNet,
    BasicBlock,
    Bottleneck,
    resnet18,
    resnet34,
    resnet50,
    resnet101,
    resnet152,
    resnext50_32x4d,
    wide_resnet50_2,
)
from .mobilenet import MobileNetV2, InvertedResidual, mobilenet_v2
from .registry import build_model, model_names

__all__ = [
    "ResNet", "BasicBlock", "Bottleneck", "build_model", "model_names",
    "resnet18", "resnet34", "resnet50", "resnet101", "resnet152",
    "resnext50_32x4d", "wide_resnet50_2",
    "MobileNetV2", "InvertedResidual", "mobilenet_v2",
]
