"""Squeeze-excite and hardswish (MobileNetV3, EfficientNet) over
``ops/csrc/se.hip``.

    y = a(x) * s[n, c],
    s = gate(W2 . hidden_act(W1 . mean_hw(a(x)) + b1) + b2)

``hidden_act`` is "relu" or "silu", ``gate`` is "hardsigmoid" or "sigmoid":
MobileNetV3 uses the first of each (the defaults), EfficientNet the second.

``a`` is the identity (``pre_act="none"``: ``x`` is already activated) or
hardswish (``pre_act="hardswish"``: ``x`` is the linear BN output and the
activation happens inside the SE kernels, never written on its own).

On the GPU, inside the kernels' contract (bf16/fp16 activations,
C % 8 == 0, C <= 4096, 1 <= Cs <= 1024), one ``autograd.Function`` runs the
seven kernels: squeeze, excite, scale forward; reduce, excite-backward,
weight gradients, apply backward.  On the CPU, with the extension off,
outside the contract or with ``AMDTRAIN_SE=0`` (A/B measurement; read on
every call) the same function is composed from plain torch ops, in fp32 for
the statistics and the MLP and without any 1x1 ``conv2d``.
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._ext import require_ext, use_ext_for
from .conv import _rows

__all__ = ["hardswish", "squeeze_excite", "SqueezeExcite"]

_PRE_ACTS = ("none", "hardswish")
_HIDDEN_ACTS = ("relu", "silu")    # the kernels' integer codes, in order
_GATES = ("hardsigmoid", "sigmoid")
_ACT_DTYPES = (torch.bfloat16, torch.float16)


def _se_enabled() -> bool:
    """AMDTRAIN_SE=0 sends squeeze-excite and hardswish to the torch ops."""
    return os.environ.get("AMDTRAIN_SE", "1") == "1"


def _on_kernels(x: torch.Tensor) -> bool:
    return _se_enabled() and x.dtype in _ACT_DTYPES and use_ext_for(x)


class _Hardswish(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x: torch.Tensor):
        ctx.save_for_backward(x)
        return require_ext().hardswish_fwd(x)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor):
        (x,) = ctx.saved_tensors
        if grad_y.stride() != x.stride() or grad_y.dtype != x.dtype:
            # the kernel walks both flat: bring the gradient to x's order
            grad_y = torch.empty_like(x).copy_(grad_y)
        return require_ext().hardswish_bwd(grad_y, x)


def hardswish(x: torch.Tensor) -> torch.Tensor:
    """``x * relu6(x + 3) / 6``: the flat vectorised kernel pair on the GPU
    (bf16/fp16; row-major and channels_last layouts are kept), else
    ``F.hardswish``."""
    if _on_kernels(x):
        if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(
                memory_format=torch.channels_last))):
            x = x.contiguous()
        return _Hardswish.apply(x)
    return F.hardswish(x)


class _SEFunction(torch.autograd.Function):
    """The seven kernels of se.hip.  Saves x as rows and the fp32 gate, mean
    and hidden activations [N, C] / [N, Cs] (under a SiLU hidden layer also
    its pre-activations, for the slope); the backward reads x and dy twice
    each (reduce, apply) and writes dx once."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")
    def forward(ctx, x, w1, b1, w2, b2, hswish: bool, hidden: int = 0,
                gate: int = 0):
        e = require_ext()
        n, c, h, w = x.shape
        cs = w1.shape[0]
        x2d = _rows(x.contiguous(memory_format=torch.channels_last))
        w1m = w1.reshape(cs, c).contiguous()
        w2m = w2.reshape(c, cs).contiguous()
        part = e.se_squeeze(x2d, n, h * w, hswish, 0)
        # {s, mean, h} and, under SiLU, z1: the tensor the hidden slope is
        # taken from is the last one either way
        out = e.se_excite(part, h * w, w1m, b1.contiguous(), w2m,
                          b2.contiguous(), hidden, gate)
        (s, mean, hid), slope_src = out[:3], out[-1]
        y2d = e.se_scale(x2d, s, n, h * w, hswish)
        ctx.save_for_backward(x2d, s, mean, hid, slope_src, w1m, w2m)
        ctx.meta = (n, c, h, w, hswish, w1.shape, w2.shape, hidden, gate)
        return y2d.view(n, h, w, c).permute(0, 3, 1, 2)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor):
        e = require_ext()
        x2d, s, mean, hid, slope_src, w1m, w2m = ctx.saved_tensors
        n, c, h, w, hswish, w1_shape, w2_shape, hidden, gate = ctx.meta
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(x2d.dtype)
        ds_part = e.se_bwd_reduce(gy2d, x2d, n, h * w, hswish, 0)
        dz2, dz1, dm = e.se_excite_bwd(ds_part, s, slope_src, w1m, w2m,
                                       h * w, hidden, gate)
        dw1, db1, dw2, db2 = e.se_wgrad(dz2, dz1, mean, hid)
        dx2d = e.se_bwd_apply(gy2d, x2d, s, dm, n, h * w, hswish)
        dx = dx2d.view(n, h, w, c).permute(0, 3, 1, 2)
        return (dx, dw1.view(w1_shape), db1, dw2.view(w2_shape), db2, None,
                None, None)


def _se_kernels(x, w1, b1, w2, b2, hswish: bool, hidden: int = 0,
                gate: int = 0) -> torch.Tensor:
    return _SEFunction.apply(x, w1, b1, w2, b2, hswish, hidden, gate)


def _se_torch(x, w1, b1, w2, b2, pre_act: str, hidden_act: str = "relu",
              gate: str = "hardsigmoid") -> torch.Tensor:
    """Plain torch ops; statistics and MLP in fp32 whatever autocast says."""
    c, cs = x.shape[1], w1.shape[0]
    hid_fn = F.silu if hidden_act == "silu" else F.relu
    gate_fn = torch.sigmoid if gate == "sigmoid" else F.hardsigmoid
    with torch.autocast(x.device.type, enabled=False):
        a = F.hardswish(x) if pre_act == "hardswish" else x
        m = a.float().mean((2, 3))
        hid = hid_fn(F.linear(m, w1.reshape(cs, c).float(), b1.float()))
        s = gate_fn(F.linear(hid, w2.reshape(c, cs).float(), b2.float()))
        return (a.float() * s[:, :, None, None]).to(x.dtype)


def _check_acts(who: str, pre_act: str, hidden_act: str, gate: str) -> None:
    for name, value, choices in (("pre_act", pre_act, _PRE_ACTS),
                                 ("hidden_act", hidden_act, _HIDDEN_ACTS),
                                 ("gate", gate, _GATES)):
        if value not in choices:
            raise ValueError(f"{who}: {name} must be one of {choices}")


def squeeze_excite(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                   w2: torch.Tensor, b2: torch.Tensor,
                   pre_act: str = "none", hidden_act: str = "relu",
                   gate: str = "hardsigmoid") -> torch.Tensor:
    """Squeeze-excite of ``x`` [N, C, H, W] with ``w1`` [Cs, C] (or
    [Cs, C, 1, 1]), ``b1`` [Cs], ``w2`` [C, Cs] (or [C, Cs, 1, 1]),
    ``b2`` [C]; see the module docstring for ``pre_act``, ``hidden_act``,
    ``gate`` and the routing."""
    _check_acts("squeeze_excite", pre_act, hidden_act, gate)
    c, cs = x.shape[1], w1.shape[0]
    if w1.numel() != cs * c or w2.numel() != cs * c or w2.shape[0] != c \
            or b1.numel() != cs or b2.numel() != c:
        raise ValueError("squeeze_excite: weight shapes do not match x")
    if (x.dim() == 4 and _on_kernels(x) and c % 8 == 0 and c <= 4096
            and 1 <= cs <= 1024 and x.shape[2] * x.shape[3] >= 1):
        # fp32 parameters go in as they are; anything else is cast here
        return _se_kernels(x, w1.float(), b1.float(), w2.float(),
                           b2.float(), pre_act == "hardswish",
                           _HIDDEN_ACTS.index(hidden_act), _GATES.index(gate))
    return _se_torch(x, w1, b1, w2, b2, pre_act, hidden_act, gate)


class SqueezeExcite(nn.Module):
    """Squeeze-excite block, by default with ReLU inside and a hardsigmoid
    gate (``hidden_act="silu", gate="sigmoid"``: EfficientNet's).  ``fc1`` and
    ``fc2`` are 1x1 ``nn.Conv2d`` modules, so the ``state_dict`` keys and
    shapes are those of torchvision's ``SqueezeExcitation``; they are never
    run as convs."""

    def __init__(self, channels: int, squeeze_channels: int,
                 pre_act: str = "none", hidden_act: str = "relu",
                 gate: str = "hardsigmoid"):
        super().__init__()
        _check_acts("SqueezeExcite", pre_act, hidden_act, gate)
        self.pre_act = pre_act
        self.hidden_act = hidden_act
        self.gate = gate
        self.fc1 = nn.Conv2d(channels, squeeze_channels, 1)
        self.fc2 = nn.Conv2d(squeeze_channels, channels, 1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return squeeze_excite(x, self.fc1.weight, self.fc1.bias,
                              self.fc2.weight, self.fc2.bias, self.pre_act,
                              self.hidden_act, self.gate)
