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
    resnext101_32x8d,
    resnext101_64x4d,
    wide_resnet50_2,
)
from .mobilenet import MobileNetV2, InvertedResidual, mobilenet_v2
from .mnasnet import (MNASNet, mnasnet0_5, mnasnet0_75, mnasnet1_0,
                      mnasnet1_3)
from .mobilenetv3 import MobileNetV3, mobilenet_v3_large, mobilenet_v3_small
from .efficientnet import EfficientNet, MBConv, efficientnet_b0
from .registry import build_model, model_names

__all__ = [
    "ResNet", "BasicBlock", "Bottleneck", "build_model", "model_names",
    "resnet18", "resnet34", "resnet50", "resnet101", "resnet152",
    "resnext50_32x4d", "resnext101_32x8d", "resnext101_64x4d",
    "wide_resnet50_2",
    "MobileNetV2", "InvertedResidual", "mobilenet_v2",
    "MNASNet", "mnasnet0_5", "mnasnet0_75", "mnasnet1_0", "mnasnet1_3",
    "MobileNetV3", "mobilenet_v3_large", "mobilenet_v3_small",
    "EfficientNet", "MBConv", "efficientnet_b0",
]
