"""Model-facing fused NHWC ops: BatchNorm(+add)(+ReLU/ReLU6), pooling.

The reference runs BN and ReLU as separate cuDNN/elementwise kernels after
every conv (53 BN layers in ResNet-50) — on MI355X that is pure
HBM traffic, so normalization, the residual add and the activation are fused
into single NHWC HIP kernels (ops/csrc/batchnorm.hip, pool.hip).  Stats are
accumulated in fp32 regardless of the activation dtype (bf16 path).

CPU fallback composes plain torch ops (autograd handled by torch); GPU path
uses custom autograd.Functions over the extension.
"""

from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from ._ext import require_ext, use_ext_for
from .conv import GradCell, _dsgrad_compact_enabled

__all__ = ["batch_norm", "bn_relu6_fusable", "bn_add_relu", "bn_add_relu_downsample",
           "bn_relu_max_pool", "max_pool_3x3_s2", "global_avg_pool"]


class _BNFunction(torch.autograd.Function):
    """Fused BN(+add)(+ReLU/ReLU6) training-mode forward/backward on NHWC
    GPU tensors.  When the producing conv attached per-block statistics
    partials (conv epilogue fusion), the reduce pass over x is skipped."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, relu, addend, parts, res_cell=None,
                relu6=False):
        e = require_ext()
        if parts is not None:
            y, mean, invstd, scale, shift, mask = \
                e.batch_norm_fwd_train_from_parts(
                    x, parts, weight, bias, running_mean, running_var,
                    float(momentum), float(eps), bool(relu), addend,
                    bool(relu6))
        else:
            y, mean, invstd, scale, shift, mask = e.batch_norm_fwd_train(
                x, weight, bias, running_mean, running_var,
                float(momentum), float(eps), bool(relu), addend,
                bool(relu6))
        # scale/shift ([C] fp32) let the bwd recompute the relu mask as
        # scale*x+shift>0 for addend-free BNs; block-tail BNs save the
        # fwd-computed 1-bit relu mask instead (bwd skips the y read)
        ctx.save_for_backward(x, y, weight, mean, invstd, scale, shift,
                              mask)
        ctx.relu = bool(relu)
        ctx.relu6 = bool(relu6)
        ctx.has_addend = addend is not None
        # block-tail BN grad mailbox (see batch_norm below): our backward
        # folds a rerouted shortcut gradient into the reduce as a second
        # linear go operand, replacing the eager CUDAFunctor_add at the
        # output's AccumulateGrad.
        ctx.res_cell = res_cell
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, y, weight, mean, invstd, scale, shift, mask = ctx.saved_tensors
        e = require_ext()
        go2, compact = None, False
        cell = getattr(ctx, "res_cell", None)
        if cell is not None and cell.g is not None:
            if cell.meta is not None:
                # compact [N*ho*wo, C] dgrad of the next block's stride-2
                # downsample conv: the reduce reads it at the even positions
                go2, compact = cell.g.contiguous(), True
            else:
                go2 = cell.g.contiguous(memory_format=torch.channels_last)
            cell.g = None
            cell.meta = None
        grad_x, grad_w, grad_b, ghat = e.batch_norm_bwd(
            x, grad_out.contiguous(memory_format=torch.channels_last),
            y, weight, mean, invstd, ctx.relu, ctx.has_addend,
            scale, shift, go2, mask, compact, ctx.relu6)
        grad_addend = ghat if ctx.has_addend else None
        return (grad_x, grad_w, grad_b, None, None, None, None, None,
                grad_addend, None, None, None)


def _bn_torch(x: torch.Tensor, bn, relu: bool,
              addend: Optional[torch.Tensor],
              relu6: bool = False) -> torch.Tensor:
    """Plain-torch reference path (CPU, or GPU with ext disabled)."""
    # match nn.BatchNorm2d bookkeeping (num_batches_tracked handled by caller)
    y = F.batch_norm(
        x, bn.running_mean, bn.running_var, bn.weight, bn.bias,
        bn.training or not bn.track_running_stats,
        bn.momentum if bn.momentum is not None else 0.0, bn.eps)
    if addend is not None:
        y = y + addend
    if relu:
        y = F.relu(y, inplace=True)
    if relu6:
        y = F.relu6(y)
    return y


def _anyc_ok(x: torch.Tensor) -> bool:
    """The any-C kernels' channel contract: whole 16-byte packs, at most 256
    of them per row (one channel group per thread of a block)."""
    C = x.size(1)
    vec = 16 // x.element_size()
    return C > 0 and C % vec == 0 and C // vec <= 256


def bn_relu6_fusable(x: torch.Tensor) -> bool:
    """Whether ``batch_norm(x, bn, relu6=True)`` has a path for ``x``: always
    off the extension (plain torch ops), on it only inside the any-C
    kernels' channel contract."""
    return not use_ext_for(x) or _anyc_ok(x)


def batch_norm(x: torch.Tensor, bn, relu: bool = False,
               addend: Optional[torch.Tensor] = None,
               relu6: bool = False) -> torch.Tensor:
    """BatchNorm2d through module ``bn``'s parameters/buffers, optionally fused
    with a residual add and/or ReLU, or with ReLU6 (no addend).

    On the GPU a power-of-two C without ReLU6 runs on the kernels it always
    did.  Any other C inside ``_anyc_ok``, and every ReLU6, runs on the any-C
    kernels, except ReLU with an addend (the block tail, power-of-two
    only).  Without ReLU6, what is left takes the library BN as it always
    did.  ReLU6 outside ``_anyc_ok`` (C % VEC != 0, or more than 256 packs
    per row such as fp32 C = 1280) has no kernel and is an error here, not a
    library composition: see ``bn_relu6_fusable``."""
    if relu and relu6:
        raise ValueError("batch_norm: relu and relu6 are mutually exclusive")
    if relu6 and addend is not None:
        raise ValueError("batch_norm: relu6 with an addend is not supported")
    C = x.size(1)
    pow2 = (C & (C - 1)) == 0
    on_ext = use_ext_for(x)
    if on_ext and relu6 and not _anyc_ok(x):
        raise NotImplementedError(
            f"batch_norm: no ReLU6 kernel for C = {C} in {x.dtype} (needs "
            f"whole 16-byte packs, at most 256 per row)")
    if on_ext and not pow2:
        on_ext = _anyc_ok(x) and not (relu and addend is not None)
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if on_ext:
        parts = getattr(x, "_amdtrain_bn_stats", None) if bn.training else None
        xc = x.contiguous(memory_format=torch.channels_last)
        ac = None if addend is None else addend.contiguous(memory_format=torch.channels_last)
        if bn.training:
            # block-tail BNs publish a mailbox the NEXT residual block can
            # reroute its shortcut gradient into (ResidualGradTap)
            cell = GradCell() if (relu and ac is not None) else None
            if cell is not None:
                # this backward's reduce also takes the next block's
                # stride-2 downsample dgrad in compact form
                cell.compact_ok = (_dsgrad_compact_enabled()
                                   and _vec_ok(xc, 256))
            out = _BNFunction.apply(xc, bn.weight, bn.bias, bn.running_mean,
                                    bn.running_var, bn.momentum, bn.eps,
                                    relu, ac, parts, cell, relu6)
            if cell is not None:
                out._amdtrain_next_cell = cell
            return out
        return require_ext().batch_norm_fwd_eval(
            xc, bn.weight, bn.bias, bn.running_mean, bn.running_var,
            float(bn.eps), bool(relu), ac, bool(relu6))
    return _bn_torch(x, bn, relu, addend, relu6)


def bn_add_relu(x: torch.Tensor, bn, addend: torch.Tensor) -> torch.Tensor:
    """relu(bn(x) + addend) — the residual-block tail, one kernel on GPU."""
    return batch_norm(x, bn, relu=True, addend=addend)


class _BNDualFunction(torch.autograd.Function):
    """Downsample-block tail: relu(bn3(x3) + bn_d(x_d)) with the downsample
    BN's output never written to memory, and one backward reduce + one
    backward apply serving both BNs (they share ghat).  Bitwise equal to
    _BNFunction(bn_d) feeding _BNFunction(bn3, addend)."""

    @staticmethod
    def forward(ctx, x3, x_d, weight3, bias3, running_mean3, running_var3,
                momentum3, eps3, weight_d, bias_d, running_mean_d,
                running_var_d, momentum_d, eps_d, parts3, parts_d, res_cell):
        e = require_ext()
        y, mean3, invstd3, mean_d, invstd_d, mask = \
            e.batch_norm_dual_fwd_train(
                x3, x_d, parts3, parts_d,
                weight3, bias3, running_mean3, running_var3,
                float(momentum3), float(eps3),
                weight_d, bias_d, running_mean_d, running_var_d,
                float(momentum_d), float(eps_d))
        ctx.save_for_backward(x3, x_d, weight3, mean3, invstd3, weight_d,
                              mean_d, invstd_d, mask)
        # same mailbox as _BNFunction block tails: the next block's rerouted
        # shortcut gradient arrives as a second go operand of the reduce
        ctx.res_cell = res_cell
        return y

    @staticmethod
    def backward(ctx, grad_out):
        (x3, x_d, weight3, mean3, invstd3, weight_d, mean_d, invstd_d,
         mask) = ctx.saved_tensors
        e = require_ext()
        go2 = None
        cell = getattr(ctx, "res_cell", None)
        if cell is not None and cell.g is not None:
            go2 = cell.g.contiguous(memory_format=torch.channels_last)
            cell.g = None
        gx3, gw3, gb3, gx_d, gw_d, gb_d = e.batch_norm_dual_bwd(
            x3, x_d, grad_out.contiguous(memory_format=torch.channels_last),
            go2, mask, weight3, mean3, invstd3, weight_d, mean_d, invstd_d)
        return (gx3, gx_d, gw3, gb3, None, None, None, None, gw_d, gb_d,
                None, None, None, None, None, None, None)


def _dsfuse_enabled() -> bool:
    """AMDTRAIN_DSFUSE=0 restores the separate downsample-BN passes."""
    return os.environ.get("AMDTRAIN_DSFUSE", "1") == "1"


def _stemfuse_enabled() -> bool:
    """AMDTRAIN_STEMFUSE=0 restores the separate stem BN+ReLU apply."""
    return os.environ.get("AMDTRAIN_STEMFUSE", "1") == "1"


def _poolbwd_fuse_enabled() -> bool:
    """AMDTRAIN_POOLBWD_FUSE=0 restores the separate stem pool backward
    (and the eager add of the pool output's two gradients)."""
    return os.environ.get("AMDTRAIN_POOLBWD_FUSE", "1") == "1"


def _vec_ok(x: torch.Tensor, max_groups: int) -> bool:
    """The kernels' channel guards: pow2 C, whole 16-byte packs, and at most
    ``max_groups`` packs per row."""
    C = x.size(1)
    vec = 16 // x.element_size()
    return (C & (C - 1)) == 0 and C % vec == 0 and C // vec <= max_groups


def bn_add_relu_downsample(x3: torch.Tensor, bn3, x_d: torch.Tensor,
                           bn_d) -> torch.Tensor:
    """relu(bn3(x3) + bn_d(x_d)) — the tail of a residual block whose
    shortcut is conv -> BN; ``x_d`` is the raw downsample-conv output.  One
    dual-BN kernel per pass in training on GPU; otherwise (eval, CPU,
    extension off, AMDTRAIN_DSFUSE=0, or a channel count the dual kernels
    do not take, e.g. fp32 C=2048) the two-BN composition."""
    if (bn3.training and bn_d.training and _dsfuse_enabled()
            and use_ext_for(x3) and x3.shape == x_d.shape
            and x3.dtype == x_d.dtype and _vec_ok(x3, 256)):
        for bn in (bn_d, bn3):
            if bn.track_running_stats and bn.num_batches_tracked is not None:
                bn.num_batches_tracked.add_(1)
        parts3 = getattr(x3, "_amdtrain_bn_stats", None)
        parts_d = getattr(x_d, "_amdtrain_bn_stats", None)
        cell = GradCell()
        out = _BNDualFunction.apply(
            x3.contiguous(memory_format=torch.channels_last),
            x_d.contiguous(memory_format=torch.channels_last),
            bn3.weight, bn3.bias, bn3.running_mean, bn3.running_var,
            bn3.momentum, bn3.eps, bn_d.weight, bn_d.bias,
            bn_d.running_mean, bn_d.running_var, bn_d.momentum, bn_d.eps,
            parts3, parts_d, cell)
        out._amdtrain_next_cell = cell
        return out
    return bn_add_relu(x3, bn3, batch_norm(x_d, bn_d))


class _MaxPool3x3S2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        e = require_ext()
        y, idx = e.max_pool_3x3_s2_fwd(x)
        ctx.save_for_backward(idx)
        ctx.in_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        e = require_ext()
        n, c, h, w = ctx.in_shape
        gx = e.max_pool_3x3_s2_bwd(
            grad_out.contiguous(memory_format=torch.channels_last), idx,
            int(h), int(w))
        return gx


def max_pool_3x3_s2(x: torch.Tensor) -> torch.Tensor:
    """3x3 stride-2 pad-1 max pool (the ResNet stem pool)."""
    if use_ext_for(x):
        return _MaxPool3x3S2.apply(x.contiguous(memory_format=torch.channels_last))
    return F.max_pool2d(x, kernel_size=3, stride=2, padding=1)


class _BNReLUMaxPool(torch.autograd.Function):
    """Stem: max_pool_3x3_s2(relu(bn(x))) with BN+ReLU applied per tap inside
    the pool kernel, so the 112x112x64 activation is neither written nor
    saved.  Backward is the BN backward in its affine-mask form, which
    recomputes the ReLU mask from scale/shift, with the pool's backward
    gather folded into its two kernels (``res_cell`` given): the
    112x112x64 gradient is never written either, and the gradient of the
    pool output's second consumer arrives through the cell instead of an
    eager add.  Without a cell: pool backward, then BN backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps, parts, res_cell=None):
        e = require_ext()
        mean, invstd, scale, shift = e.batch_norm_train_stats(
            x, parts, weight, bias, running_mean, running_var,
            float(momentum), float(eps))
        y, idx = e.max_pool_3x3_s2_fwd(x, scale, shift)
        ctx.save_for_backward(x, idx, weight, mean, invstd, scale, shift)
        ctx.res_cell = res_cell
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, idx, weight, mean, invstd, scale, shift = ctx.saved_tensors
        e = require_ext()
        go = grad_out.contiguous(memory_format=torch.channels_last)
        cell = getattr(ctx, "res_cell", None)
        if cell is not None:
            go2 = None
            if cell.g is not None:
                go2 = cell.g.to(go.dtype).contiguous(
                    memory_format=torch.channels_last)
                cell.g = None
            grad_x, grad_w, grad_b = e.batch_norm_bwd_pool(
                x, go, go2, idx, weight, mean, invstd, scale, shift)
        else:
            gp = e.max_pool_3x3_s2_bwd(go, idx, int(x.size(2)),
                                       int(x.size(3)))
            grad_x, grad_w, grad_b, _ = e.batch_norm_bwd(
                x, gp, None, weight, mean, invstd, True, False, scale,
                shift, None, None)
        return grad_x, grad_w, grad_b, None, None, None, None, None, None


def bn_relu_max_pool(x: torch.Tensor, bn) -> torch.Tensor:
    """max_pool_3x3_s2(relu(bn(x))) — the ResNet stem after conv1.  One
    fused pool kernel in training on GPU; otherwise (eval, CPU, extension
    off, AMDTRAIN_STEMFUSE=0) the two-op composition."""
    if (bn.training and _stemfuse_enabled() and use_ext_for(x)
            and _vec_ok(x, 512)):
        if bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        parts = getattr(x, "_amdtrain_bn_stats", None)
        # the pool-gather backward is register-path only (C/VEC <= 256); it
        # also publishes the mailbox the first block's ResidualGradTap
        # reroutes the pool output's second gradient into
        cell = GradCell() if (_poolbwd_fuse_enabled()
                              and _vec_ok(x, 256)) else None
        out = _BNReLUMaxPool.apply(
            x.contiguous(memory_format=torch.channels_last), bn.weight,
            bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
            parts, cell)
        if cell is not None:
            out._amdtrain_next_cell = cell
        return out
    return max_pool_3x3_s2(batch_norm(x, bn, relu=True))


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        e = require_ext()
        y = e.global_avg_pool_fwd(x)
        ctx.in_shape = x.shape
        return y

    @staticmethod
    def backward(ctx, grad_out):
        e = require_ext()
        n, c, h, w = ctx.in_shape
        return e.global_avg_pool_bwd(grad_out.contiguous(), int(h), int(w))


def global_avg_pool(x: torch.Tensor) -> torch.Tensor:
    """Global average pool to [N,C,1,1] (AdaptiveAvgPool2d((1,1)) parity)."""
    if use_ext_for(x):
        return _GlobalAvgPool.apply(x.contiguous(memory_format=torch.channels_last))
    return F.adaptive_avg_pool2d(x, (1, 1))
