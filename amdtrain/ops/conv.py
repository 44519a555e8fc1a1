"""Hand-written convolutions over the gfx950 MFMA GEMM kernels.

A 1x1 conv on NHWC data is exactly a GEMM over rows R = N*H*W
(SURVEY §2c): forward C[R,Cout] = X[R,Cin] x W[Cout,Cin]^T, dgrad uses the
pre-transposed weight.  Strided (downsample) 1x1 convs gather/scatter the
even rows around the same GEMMs.  3x3, grouped 3x3 and the generic (stem)
convs are implicit GEMMs over the same tiles.  Stride-1 1x1 convs with thin
channel counts off the 32 grid (MobileNetV2's 16, 24, 144) run the same
product on the skinny-GEMM kernel of pwconv.hip instead.

Every weight gradient is tn2_wgrad (wgrad.hip): one launch, split-M fp32
partials collapsed in a fixed order, so it has no atomics and is bitwise
deterministic.

Dispatch: ``AmdConv2d`` routes all eligible convs (GPU + extension + bf16
path) to the hand-written kernels; see the class docstring for the matrix.
profiles/ holds the per-shape measurements behind the defaults.
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn

from ._ext import ext_available, require_ext


def _rows(x: torch.Tensor) -> torch.Tensor:
    """channels_last NCHW -> [N*H*W, C] view (no copy)."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c)


def _fuse_stats_enabled() -> bool:
    return os.environ.get("AMDTRAIN_FUSE_BNSTATS", "1") == "1"


def _stem_s2d_enabled() -> bool:
    """Width space-to-depth form of the thin-channel 7x7 s2 stem (see
    stem_s2d_input): AMDTRAIN_STEM_S2D=1.  Off by default although it is
    the faster form (profiles/README.md): its K grouping and its
    statistics epilogue change the last bits of the stem output, and a
    training run amplifies those, so results would no longer repeat the
    49-tap path's.  The default keeps the 3->8 channel-padded 49 taps."""
    return os.environ.get("AMDTRAIN_STEM_S2D", "0") == "1"


def _stem_nt64_enabled() -> bool:
    """64-wide n-tile for the channel-padded 49-tap stem forward when
    Cout <= 64 (same K order, identical output); AMDTRAIN_STEM_NT64=0 keeps
    the 128-wide tile."""
    return os.environ.get("AMDTRAIN_STEM_NT64", "1") == "1"


def _s2parity_enabled() -> bool:
    """Parity-class tiles for the stride-2 conv3x3 dgrad (conv3x3.hip);
    AMDTRAIN_CONV3X3_S2PARITY=0 walks all 9 taps for every tile."""
    return os.environ.get("AMDTRAIN_CONV3X3_S2PARITY", "1") == "1"


def _nt64_enabled() -> bool:
    """64-wide n-tile for conv3x3 outputs of <= 64 channels;
    AMDTRAIN_CONV3X3_NT64=0 keeps the 128-wide tile."""
    return os.environ.get("AMDTRAIN_CONV3X3_NT64", "1") == "1"


def _epilogue_mode() -> int:
    """bf16 C-store epilogue of the MFMA kernels (csrc/common.h):
    AMDTRAIN_EPILOGUE=0 per-element predicated 2-byte stores, 1 lean
    addressing on interior tiles, 2 lean addressing + 16-byte stores.  All
    modes give the same bits.  Read on every call and passed down as an
    argument, so one process can compare them.  Unset -> -1: every kernel
    runs its measured default (2, except the dual-n-tile 1x1 GEMM: 1; see
    docs/KERNELS.md)."""
    v = os.environ.get("AMDTRAIN_EPILOGUE")
    if v is None or v == "":
        return -1
    mode = int(v)
    if mode not in (0, 1, 2):
        raise ValueError(f"AMDTRAIN_EPILOGUE must be 0, 1 or 2, got {v!r}")
    return mode


class GradCell:
    """Shared mailbox between ResidualGradTap and the producing block-tail
    _BNFunction (fused.py).  A plain class (NOT a dict):
    torch.amp.custom_fwd(cast_inputs=...) deep-copies dict arguments while
    casting, which would silently disconnect the mailbox.

    ``compact_ok`` is set by a producer whose backward can read a stride-2
    1x1 conv's dgrad in its compact ``[N*ho*wo, C]`` form; the conv then
    leaves that tensor in ``g`` with ``meta = (n, h, w, ho, wo)`` instead of
    scattering it to full resolution."""
    __slots__ = ("armed", "g", "compact_ok", "meta")

    def __init__(self):
        self.armed = False
        self.g = None
        self.compact_ok = False
        self.meta = None


def _dsgrad_compact_enabled() -> bool:
    """AMDTRAIN_DSGRAD_COMPACT=0 restores the scatter_rows_x2 pass."""
    return os.environ.get("AMDTRAIN_DSGRAD_COMPACT", "1") == "1"


class ResidualGradTap(torch.autograd.Function):
    """Reroutes a residual block's identity-shortcut gradient into the
    PRODUCING block-tail BN's backward (a second, linearly-read go operand
    of its reduce kernel) instead of an eager 2-read+1-write tensor add at
    the shared tensor's AccumulateGrad.

    The tap wraps the ADDEND input of block b's bn_add_relu; the cell is
    created and attached by block b-1's tail BN, whose backward runs
    strictly AFTER every node of block b (it is upstream of all of them).
    A first attempt fused this add into conv1's dgrad epilogue instead:
    measured SLOWER (the fragment-shaped 2-byte epilogue reads cost ~5x
    the eager add) — the BN reduce reads the extra operand with the same
    16 B vectorized stream as its other inputs.  Safety latch: the grad is
    stashed ONLY when the producing BN armed the cell; any fallback keeps
    plain autograd accumulation.

    A stride-2 downsample conv fed by the tap may already have left its
    compact dgrad in the cell (see _Conv1x1.backward); it then returns no
    input gradient and the tap sees ``None``.
    """

    @staticmethod
    def forward(ctx, z: torch.Tensor, cell: "GradCell"):
        ctx.cell = cell
        ctx.set_materialize_grads(False)
        return z.view_as(z)

    @staticmethod
    def backward(ctx, grad):
        if grad is None:
            return None, None
        if ctx.cell.armed:
            ctx.cell.g = grad
            ctx.cell.meta = None
            return None, None
        return grad, None


def tap_residual(x: torch.Tensor, cell: "GradCell") -> torch.Tensor:
    """ResidualGradTap on ``x``; the result also carries the cell so a
    downsample conv consuming it can find the mailbox."""
    out = ResidualGradTap.apply(x, cell)
    out._amdtrain_tap_cell = cell
    return out


class _Conv1x1(torch.autograd.Function):
    """1x1 conv; forward also emits per-block BN-statistics partials
    (non-differentiable 2nd output) for the fused conv->BN pipeline when
    stride == 1 and fusion is enabled.  An optional grad_cell (see
    ResidualGradTap) fuses the residual-branch gradient into the dgrad."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int,
                cell=None):
        e = require_ext()
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        xc = x.contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        w2d = weight.reshape(cout, cin)
        stats = None
        ctx.cell = cell
        if stride > 1:
            # even-row gather happens inside the A staging (no copy); the
            # full x2d is saved — it is the same tensor the sibling conv of
            # the residual block already saves, so no extra memory
            y2d = e.gemm_bt_strided(x2d, w2d, n, h, w, stride,
                                    _epilogue_mode())
            ho = (h + stride - 1) // stride
            wo = (w + stride - 1) // stride
        elif _fuse_stats_enabled():
            y2d, stats = e.gemm_bt_stats(x2d, w2d, _epilogue_mode())
            ho, wo = h, w
        else:
            y2d = e.gemm_bt(x2d, w2d, False, None, None,
                            _epilogue_mode())
            ho, wo = h, w
        ctx.save_for_backward(x2d, w2d)
        ctx.meta = (n, cin, h, w, stride, ho, wo, cout)
        y = y2d.view(n, ho, wo, cout).permute(0, 3, 1, 2)
        if stats is None:
            stats = torch.empty(0, device=x.device)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor, _grad_stats=None):
        e = require_ext()
        x2d, w2d = ctx.saved_tensors
        n, cin, h, w, stride, ho, wo, cout = ctx.meta
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(torch.bfloat16)
        # dgrad: dX = dY x W  (BT form with pre-transposed weight)
        wT = e.transpose_2d(w2d)                      # [Cin, Cout]
        dx2d = e.gemm_bt(gy2d, wT, False, None, None,
                         _epilogue_mode())      # [R_sub, Cin] bf16
        if stride > 1:
            cell = ctx.cell
            if (stride == 2 and cell is not None and cell.armed
                    and cell.compact_ok):
                # the producing block tail's reduce reads the compact dgrad
                # at the even positions itself: no full-resolution tensor
                # that is 3/4 zeros.  It travels out of band (autograd
                # would reject its shape as this conv's input gradient).
                cell.g = dx2d
                cell.meta = (n, h, w, ho, wo)
                dx = None
            else:
                # fused zero+scatter (one write pass; stride-2 only in
                # ResNet)
                dx = e.scatter_rows_x2(dx2d, n, h, w, ho, wo)
            dw = e.tn2_wgrad(gy2d, x2d, 1, n, h, w, stride, 1)
        else:
            dx = dx2d.view(n, ho, wo, cin).permute(0, 3, 1, 2)
            dw = e.tn2_wgrad(gy2d, x2d)
        return dx, dw.reshape(cout, cin, 1, 1), None, None


def conv1x1_mfma(x: torch.Tensor, weight: torch.Tensor,
                 stride: int = 1) -> torch.Tensor:
    # a stride-2 conv fed by a ResidualGradTap is the downsample conv: it
    # may hand its compact dgrad to the tap's mailbox
    cell = getattr(x, "_amdtrain_tap_cell", None) if stride == 2 else None
    y, stats = _Conv1x1.apply(x, weight, stride, cell)
    if stats.numel():
        y._amdtrain_bn_stats = stats
    return y


def _pwconv_enabled() -> bool:
    """Thin pointwise kernel (pwconv.hip) for stride-1 1x1 convs off the 32
    grid; AMDTRAIN_PWCONV=0 restores the routing from before it (generic
    kernel or MIOpen) for A/B measurement."""
    return os.environ.get("AMDTRAIN_PWCONV", "1") == "1"


def _pw_gemm_ok(k: int, n: int) -> bool:
    """Host contract of pw_gemm for one orientation: multiples of 8, and the
    weight zero-padded to 32 x 32 blocks fits 16 KiB of LDS."""
    return (k >= 8 and n >= 8 and k % 8 == 0 and n % 8 == 0
            and ((k + 31) // 32) * ((n + 31) // 32) <= 8)


def pw_thin_ok(cin: int, cout: int) -> bool:
    """True when a stride-1 1x1 conv cin -> cout belongs to the thin
    pointwise kernel: not on the MFMA GEMM's 32 grid, and inside pw_gemm's
    contract both as forward (K = cin, N = cout) and as input gradient
    (K = cout, N = cin).  Pure Python; needs no GPU."""
    if cin % 32 == 0 and cout % 32 == 0:
        return False
    return _pw_gemm_ok(cin, cout) and _pw_gemm_ok(cout, cin)


class _ConvPw(torch.autograd.Function):
    """Stride-1 1x1 conv with thin channel counts over pw_gemm
    (pwconv.hip): forward with the BN-statistics partials as a second,
    non-differentiable output, input gradient as the same kernel on the
    transposed weight, weight gradient as tn2_wgrad."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor):
        e = require_ext()
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        xc = x.contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        w2d = weight.reshape(cout, cin)
        y2d, stats = e.pw_gemm(x2d, w2d, _fuse_stats_enabled())
        ctx.save_for_backward(x2d, w2d)
        ctx.meta = (n, cin, h, w, cout)
        y = y2d.view(n, h, w, cout).permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor, _grad_stats=None):
        e = require_ext()
        x2d, w2d = ctx.saved_tensors
        n, cin, h, w, cout = ctx.meta
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wT = e.transpose_2d(w2d)                  # [Cin, Cout]
            dx2d = e.pw_gemm(gy2d, wT, False)[0]      # [R, Cin] bf16
            dx = dx2d.view(n, h, w, cin).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dw = e.tn2_wgrad(gy2d, x2d).reshape(cout, cin, 1, 1)
        return dx, dw


def conv1x1_thin(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """Stride-1 1x1 conv for channel counts inside ``pw_thin_ok``."""
    y, stats = _ConvPw.apply(x, weight)
    if stats.numel():
        y._amdtrain_bn_stats = stats
    return y


class _Conv3x3(torch.autograd.Function):
    """3x3 pad-1 conv (stride 1/2) over the implicit-GEMM gfx950 kernels."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int):
        e = require_ext()
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        xc = x.contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        # channels_last weight [Cout,Cin,3,3] is [Cout][kh][kw][Cin] in memory
        w2d = weight.contiguous(memory_format=torch.channels_last) \
            .permute(0, 2, 3, 1).reshape(cout, 9 * cin)
        nt64 = _nt64_enabled()
        if _fuse_stats_enabled():
            y2d, stats = e.conv3x3_fwd_stats(x2d, n, h, w, stride, w2d,
                                             False, nt64,
                                             _epilogue_mode())
        else:
            y2d = e.conv3x3_fwd(x2d, n, h, w, stride, w2d, nt64,
                                _epilogue_mode())
            stats = torch.empty(0, device=x.device)
        ctx.save_for_backward(x2d, w2d)
        ctx.meta = (n, cin, h, w, stride, cout)
        ho = (h + 2 - 3) // stride + 1
        wo = (w + 2 - 3) // stride + 1
        y = y2d.view(n, ho, wo, cout).permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor, _grad_stats=None):
        e = require_ext()
        x2d, w2d = ctx.saved_tensors
        n, cin, h, w, stride, cout = ctx.meta
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(torch.bfloat16)
        dx2d = e.conv3x3_dgrad(gy2d, n, h, w, stride, w2d, False,
                               _s2parity_enabled(), _nt64_enabled(),
                               _epilogue_mode())
        dx = dx2d.view(n, h, w, cin).permute(0, 3, 1, 2)
        # [Cout, 9*Cin] f32 — single-launch tap-gather TN (wgrad.hip)
        dw2d = e.tn2_wgrad(gy2d, x2d, 9, n, h, w, stride, 2)
        # back to [Cout,Cin,3,3] (channels_last layout of the weight)
        dw = dw2d.view(cout, 3, 3, cin).permute(0, 3, 1, 2) \
            .contiguous(memory_format=torch.channels_last)
        return dx, dw, None


def conv3x3_mfma(x: torch.Tensor, weight: torch.Tensor,
                 stride: int = 1) -> torch.Tensor:
    y, stats = _Conv3x3.apply(x, weight, stride)
    if stats.numel():
        y._amdtrain_bn_stats = stats
    return y


class _ConvGrouped3x3(torch.autograd.Function):
    """Grouped 3x3 conv (ResNeXt) as a BLOCK-DIAGONALIZED dense conv over
    the in-house implicit-GEMM kernels.

    The grouped weight [Cout, S, 3, 3] (S = Cin/groups) is expanded to a
    dense [Cout, 9*Cin] with zeros off the group diagonal, then the
    standard conv3x3 fwd/dgrad/wgrad kernels run at dense speed (~640 TF)
    — MIOpen's grouped path measured ~4x slower end-to-end on
    resnext50_32x4d.  Numerically exact: zeros cannot contaminate fwd or
    dgrad, and wgrad is an outer product, so slicing the group diagonal
    of the dense dW recovers the grouped gradient bit-for-bit.
    """

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int,
                groups: int):
        e = require_ext()
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        sg = cin // groups
        xc = x.contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        # dense [G, Sout, 3, 3, G, Sin] with the grouped weight on the
        # (g, :, :, :, g, :) diagonal
        sout = cout // groups
        wg = weight.contiguous(memory_format=torch.channels_last) \
            .permute(0, 2, 3, 1).reshape(groups, sout, 3, 3, sg)
        dense = torch.zeros(groups, sout, 3, 3, groups, sg,
                            dtype=wg.dtype, device=wg.device)
        gi = torch.arange(groups, device=wg.device)
        dense[gi, :, :, :, gi, :] = wg
        w2d = dense.reshape(cout, 3, 3, cin).reshape(cout, 9 * cin)
        # group-diagonal banding: skip the provably-zero K-steps (the
        # 128-channel window of each n-tile) when alignment allows
        banded = (cin == cout and cin % 128 == 0)
        if _fuse_stats_enabled():
            y2d, stats = e.conv3x3_fwd_stats(x2d, n, h, w, stride, w2d,
                                             banded, _nt64_enabled(),
                                             _epilogue_mode())
        else:
            y2d = e.conv3x3_fwd(x2d, n, h, w, stride, w2d, _nt64_enabled(),
                                _epilogue_mode())
            stats = torch.empty(0, device=x.device)
        ctx.save_for_backward(x2d, w2d)
        ctx.meta = (n, cin, h, w, stride, cout, groups, banded)
        ho = (h + 2 - 3) // stride + 1
        wo = (w + 2 - 3) // stride + 1
        y = y2d.view(n, ho, wo, cout).permute(0, 3, 1, 2)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor, _grad_stats=None):
        e = require_ext()
        x2d, w2d = ctx.saved_tensors
        n, cin, h, w, stride, cout, groups, banded = ctx.meta
        sg = cin // groups
        sout = cout // groups
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(torch.bfloat16)
        dx2d = e.conv3x3_dgrad(gy2d, n, h, w, stride, w2d, banded,
                               _s2parity_enabled(), _nt64_enabled(),
                               _epilogue_mode())
        dx = dx2d.view(n, h, w, cin).permute(0, 3, 1, 2)
        if banded:
            # compact band [Cout, 9, 128]: extract the group diagonal of
            # each 128-channel window
            dwb = e.tn2_wgrad_banded(gy2d, x2d, n, h, w, stride) \
                .view(cout // 128, 128 // sg, sg, 9, 128 // sg, sg)
            bi = torch.arange(cout // 128, device=dwb.device)[:, None]
            gi = torch.arange(128 // sg, device=dwb.device)[None, :]
            dw = dwb[bi, gi, :, :, gi, :].reshape(cout, 9, sg) \
                .view(cout, 3, 3, sg).permute(0, 3, 1, 2) \
                .contiguous(memory_format=torch.channels_last)
            return dx, dw, None, None
        dw2d = e.tn2_wgrad(gy2d, x2d, 9, n, h, w, stride, 2)
        # slice the group diagonal of the dense dW
        dwd = dw2d.view(groups, sout, 3, 3, groups, sg)
        gi = torch.arange(groups, device=dwd.device)
        dw = dwd[gi, :, :, :, gi, :].permute(0, 1, 4, 2, 3) \
            .reshape(cout, sg, 3, 3) \
            .contiguous(memory_format=torch.channels_last)
        return dx, dw, None, None


def conv3x3_grouped_mfma(x: torch.Tensor, weight: torch.Tensor,
                         stride: int, groups: int) -> torch.Tensor:
    y, stats = _ConvGrouped3x3.apply(x, weight, stride, groups)
    if stats.numel():
        y._amdtrain_bn_stats = stats
    return y


class _DwConv3x3(torch.autograd.Function):
    """Depthwise 3x3 pad-1 conv (stride 1/2) over the vectorised stencil
    kernels of dwconv.hip: forward, gather-form input gradient and a
    two-level fixed-order weight gradient, all NHWC bf16 with fp32
    accumulation.  The kernels take the weight tap-major, ``w9`` [9, C]."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int):
        e = require_ext()
        n, c, h, w = x.shape
        xc = x.to(torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        wb = weight.to(torch.bfloat16)
        w9 = wb.reshape(c, 9).t().contiguous()
        y2d = e.dwconv3x3_fwd(x2d, n, h, w, stride, w9)
        ctx.save_for_backward(x2d, wb)
        ctx.meta = (n, c, h, w, stride)
        ho = (h + 2 - 3) // stride + 1
        wo = (w + 2 - 3) // stride + 1
        return y2d.view(n, ho, wo, c).permute(0, 3, 1, 2)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor):
        e = require_ext()
        x2d, wb = ctx.saved_tensors
        n, c, h, w, stride = ctx.meta
        gy = grad_y.contiguous(memory_format=torch.channels_last)
        gy2d = _rows(gy).to(torch.bfloat16)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            w9 = wb.reshape(c, 9).t().contiguous()
            dx2d = e.dwconv3x3_dgrad(gy2d, n, h, w, stride, w9)
            dx = dx2d.view(n, h, w, c).permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            dw9 = e.dwconv3x3_wgrad(gy2d, x2d, n, h, w, stride)  # [9, C] f32
            dw = dw9.t().reshape(c, 1, 3, 3)
        return dx, dw, None


def dwconv3x3(x: torch.Tensor, weight: torch.Tensor,
              stride: int = 1) -> torch.Tensor:
    """Depthwise 3x3 pad-1 conv, ``weight`` [C, 1, 3, 3], stride 1 or 2.
    On the GPU with the extension loaded: the bf16 stencil kernels (C must
    be a multiple of 8).  On CPU, or with the extension off: exactly
    ``F.conv2d(..., groups=C)``."""
    if x.is_cuda and ext_available():
        return _DwConv3x3.apply(x, weight, stride)
    return torch.nn.functional.conv2d(x, weight, None, stride, 1, 1,
                                      x.shape[1])


def stem_s2d_input(x_nhwc: torch.Tensor) -> torch.Tensor:
    """[N, H, W, C] (C <= 4, W even) -> X' [N, H, W/2, 8]: channels padded
    to 4, then two neighbouring pixels share one 8-channel row, channel
    index p*4 + c for pixel 2*group + p.  After the pad this is a pure
    reinterpretation of the NHWC memory — no second copy."""
    n, h, w, c = x_nhwc.shape
    assert c <= 4 and w % 2 == 0
    x4 = torch.nn.functional.pad(x_nhwc, (0, 4 - c))
    return x4.reshape(n, h, w // 2, 8)


def stem_s2d_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, C, 7, 7] -> W2' [Cout, kh=7, g=4, p=2, c=4] with
    W2'[cout, kh, g, p, c] = w[cout, c, kh, 2g+p-1], zero where kw = -1 or
    c >= C.

    With X' = stem_s2d_input(x), the 7x7 stride-2 pad-3 conv of x equals
    the conv of X' with a 7 x 4 (kh x g) kernel over 8 channels, stride
    (2, 1), top padding 3 and left padding 2 groups, at the original
    Hout x Wout: input pixel 2*wo - 3 + kw is group wo - 2 + g, slot p.
    The image edges sit at even pixels, so padding comes in whole groups;
    the one zero-weight slot (g = 0, p = 0) reads real data."""
    cout, c, kh, kw = weight.shape
    assert c <= 4 and kh == 7 and kw == 7
    wp = torch.nn.functional.pad(weight, (1, 0, 0, 0, 0, 4 - c))
    return wp.permute(0, 2, 3, 1).reshape(cout, 7, 4, 2, 4)


def stem_s2d_dweight(dw2: torch.Tensor, cin: int) -> torch.Tensor:
    """Inverse index gather of stem_s2d_weight: dW2' [Cout, 224] (or any
    shape of 7*4*2*4 trailing elements) -> dW [Cout, cin, 7, 7]."""
    cout = dw2.shape[0]
    return dw2.reshape(cout, 7, 8, 4)[:, :, 1:, :cin].permute(0, 3, 1, 2)


def _stem_s2d_ok(weight: torch.Tensor, w: int, stride: int, pad: int) -> bool:
    return (weight.shape[1] <= 4 and tuple(weight.shape[2:]) == (7, 7)
            and stride == 2 and pad == 3 and w % 2 == 0)


class _ConvGeneric(torch.autograd.Function):
    """Generic implicit-GEMM conv (element-gather im2col) — serves the 7x7
    stem and any other odd configuration.  Input gradient gathers dY
    through the transposed-conv map (conv_generic_dgrad) when needed.

    ``s2d`` runs a thin-channel 7x7 s2 p3 conv in its width space-to-depth
    form (stem_s2d_weight): K = 224 instead of 416, and the forward also
    emits the BN-statistics partials (second, non-differentiable output;
    empty otherwise)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.bfloat16)
    def forward(ctx, x: torch.Tensor, weight: torch.Tensor, stride: int,
                pad: int, s2d: bool = False, nt64: bool = False):
        e = require_ext()
        n, cin, h, w = x.shape
        cout, _, kh, kw = weight.shape
        xc = x.contiguous(memory_format=torch.channels_last)
        x2d = _rows(xc)
        ho = (h + 2 * pad - kh) // stride + 1
        wo = (w + 2 * pad - kw) // stride + 1
        ctx.s2d = s2d
        if s2d:
            x8 = stem_s2d_input(x2d.view(n, h, w, cin)) \
                .view(n * h * (w // 2), 8)
            w2 = stem_s2d_weight(weight).reshape(cout, 224)
            geom = (n, h, w // 2, 7, 4, 2, 3, w2, 1, 2, ho, wo, True,
                    _epilogue_mode())
            if _fuse_stats_enabled():
                y2d, stats = e.conv_generic_fwd_stats(x8, *geom)
            else:
                y2d = e.conv_generic_fwd(x8, *geom)
                stats = torch.empty(0, device=x.device)
            ctx.save_for_backward(x8, weight)
            ctx.meta = (n, cin, h, w, kh, kw, stride, pad, cout, 224, 8)
            ctx.mark_non_differentiable(stats)
            return y2d.view(n, ho, wo, cout).permute(0, 3, 1, 2), stats
        w4 = weight.contiguous(memory_format=torch.channels_last) \
            .permute(0, 2, 3, 1)                       # [Cout, KH, KW, Cin]
        if cin < 8:
            # stem fast path: pad channels to 8 so every 16 B staging unit
            # is one tap — the kernel's vectorized tap-gather (C8) route
            x2d = torch.nn.functional.pad(x2d, (0, 8 - cin))
            w4 = torch.nn.functional.pad(w4, (0, 8 - cin))
            cin_k = 8
        else:
            cin_k = cin
        k = kh * kw * cin_k
        kpad = (k + 31) // 32 * 32
        w2 = w4.reshape(cout, k)
        if kpad != k:
            w2 = torch.nn.functional.pad(w2, (0, kpad - k))
        y2d = e.conv_generic_fwd(x2d, n, h, w, kh, kw, stride, pad, w2,
                                 0, -1, 0, 0, nt64, _epilogue_mode())
        ctx.save_for_backward(x2d, weight)
        ctx.meta = (n, cin, h, w, kh, kw, stride, pad, cout, k, cin_k)
        stats = torch.empty(0, device=x.device)
        ctx.mark_non_differentiable(stats)
        return y2d.view(n, ho, wo, cout).permute(0, 3, 1, 2), stats

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_y: torch.Tensor, _grad_stats=None):
        e = require_ext()
        x2d, weight = ctx.saved_tensors
        n, cin, h, w, kh, kw, stride, pad, cout, k, cin_k = ctx.meta
        gy2d = _rows(grad_y.contiguous(memory_format=torch.channels_last)) \
            .to(torch.bfloat16)
        dx = None
        if ctx.needs_input_grad[0]:
            # weight permuted [Cin, KH*KW*Cout] + K2 padding
            k2 = kh * kw * cout
            k2p = (k2 + 31) // 32 * 32
            w2p = weight.to(torch.bfloat16).permute(1, 2, 3, 0) \
                .reshape(cin, k2)
            if k2p != k2:
                w2p = torch.nn.functional.pad(w2p, (0, k2p - k2))
            dx2d = e.conv_generic_dgrad(gy2d, w2p.contiguous(), n, h, w,
                                        kh, kw, stride, pad)
            dx = dx2d.view(n, h, w, cin).permute(0, 3, 1, 2)
        if ctx.s2d:
            # x2d is X' [N*H*(W/2), 8]: 28 taps of 8 channels, so K' = 224
            # sits in one k-tile and dY is staged once
            ho = (h + 2 * pad - kh) // stride + 1
            wo = (w + 2 * pad - kw) // stride + 1
            dwp = e.tn2_wgrad(gy2d, x2d, 28, n, h, w // 2, 2, 2, 7, 4, 3,
                              1, 2, ho, wo)              # [Cout, 224] f32
            dw = stem_s2d_dweight(dwp, cin) \
                .contiguous(memory_format=torch.channels_last)
        else:
            # tap-gather TN core; x2d is already channel-padded (fwd)
            dwp = e.tn2_wgrad(gy2d, x2d, kh * kw, n, h, w, stride, 2,
                              kh, kw, pad)               # [Cout, taps*cin_k]
            dw = dwp.view(cout, kh * kw, cin_k)[:, :, :cin] \
                .view(cout, kh, kw, cin).permute(0, 3, 1, 2) \
                .contiguous(memory_format=torch.channels_last)
        return dx, dw, None, None, None, None


def conv_stem_mfma(x: torch.Tensor, weight: torch.Tensor, stride: int,
                   pad: int) -> torch.Tensor:
    """Generic-path conv (the 7x7 stem and odd configurations).  The weight
    gradient is the tap-gather tn2_wgrad, which needs ``cout % 8 == 0``
    (``AmdConv2d`` only routes ``out_channels % 16 == 0`` here); a direct
    caller with another ``cout`` gets tn2_wgrad's error in backward."""
    s2d = (_stem_s2d_enabled()
           and _stem_s2d_ok(weight, x.shape[3], stride, pad))
    y, stats = _ConvGeneric.apply(x, weight, stride, pad, s2d,
                                  _stem_nt64_enabled())
    if stats.numel():
        y._amdtrain_bn_stats = stats
    return y


def _conv1x1_env_default() -> str:
    return os.environ.get("AMDTRAIN_CONV1X1", "custom")


class AmdConv2d(nn.Conv2d):
    """nn.Conv2d dispatching to the hand-written gfx950 kernels.

    State dict / init are identical to nn.Conv2d.  On-GPU bf16 paths:
    1x1 -> MFMA GEMM (gemm.hip), or, stride 1 with channel counts off the
    32 grid but inside ``pw_thin_ok``, the thin pointwise kernel
    (pwconv.hip; AMDTRAIN_PWCONV=0 restores the routing from before it),
    3x3 pad-1 s1/s2 -> implicit GEMM
    (conv3x3.hip), anything else without an input gradient (the 7x7
    stem) -> generic element-gather implicit GEMM (conv_stem.hip).
    Depthwise 3x3 pad-1 s1/s2 (groups == in == out channels, C % 8 == 0)
    -> vectorised stencil (dwconv.hip); other grouped 3x3 with
    in % 32 == 0 and out % 16 == 0 (ResNeXt) -> block-diagonalized dense
    conv3x3.  Every other grouped conv, dilated convs, convs with a bias
    and fp32 inference fall through to MIOpen.
    Env overrides AMDTRAIN_CONV1X1 / AMDTRAIN_CONV3X3 / AMDTRAIN_CONV3X3G /
    AMDTRAIN_CONVSTEM / AMDTRAIN_DWCONV = "miopen" for A/B measurement,
    read on every call.
    """

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # MFMA path is bf16: eligible under autocast or with bf16 inputs;
        # fp32 inference/training falls through to MIOpen
        bf16_ok = (x.dtype == torch.bfloat16
                   or torch.is_autocast_enabled("cuda"))
        if (x.is_cuda and bf16_ok and ext_available()
                and self.bias is None and self.dilation == (1, 1)
                and self.groups > 1):
            # depthwise 3x3: vectorised stencil, not a GEMM
            if (self.groups == self.in_channels == self.out_channels
                    and self.kernel_size == (3, 3)
                    and self.padding == (1, 1)
                    and self.stride in ((1, 1), (2, 2))
                    and self.in_channels % 8 == 0):
                if os.environ.get("AMDTRAIN_DWCONV", "custom") == "miopen":
                    return super().forward(x)
                return dwconv3x3(x, self.weight, self.stride[0])
            # grouped 3x3 (ResNeXt): block-diagonalized dense path
            if (self.kernel_size == (3, 3) and self.padding == (1, 1)
                    and self.stride[0] in (1, 2)
                    and self.in_channels % 32 == 0
                    and self.out_channels % 16 == 0
                    and self.in_channels % self.groups == 0
                    and os.environ.get("AMDTRAIN_CONV3X3G", "custom")
                    == "custom"):
                return conv3x3_grouped_mfma(x, self.weight, self.stride[0],
                                            self.groups)
            return super().forward(x)
        if (x.is_cuda and bf16_ok and ext_available()
                and self.bias is None and self.groups == 1
                and self.dilation == (1, 1)):
            ch_ok = (self.in_channels % 32 == 0
                     and self.out_channels % 16 == 0)
            # thin pointwise: stride-1 1x1 off the 32 grid (pw_thin_ok is
            # false on it, so every 32-grid layer keeps the GEMM below)
            if (self.kernel_size == (1, 1) and self.padding == (0, 0)
                    and self.stride == (1, 1)
                    and pw_thin_ok(self.in_channels, self.out_channels)
                    and _pwconv_enabled()
                    and _conv1x1_env_default() == "custom"):
                return conv1x1_thin(x, self.weight)
            if (ch_ok and self.kernel_size == (1, 1)
                    and self.padding == (0, 0)
                    and _conv1x1_env_default() == "custom"):
                return conv1x1_mfma(x, self.weight, self.stride[0])
            if (ch_ok and self.kernel_size == (3, 3)
                    and self.padding == (1, 1)
                    and self.stride[0] in (1, 2)
                    and os.environ.get("AMDTRAIN_CONV3X3", "custom")
                    == "custom"):
                return conv3x3_mfma(x, self.weight, self.stride[0])
            if (self.out_channels % 16 == 0
                    and self.stride[0] == self.stride[1]
                    and self.padding[0] == self.padding[1]
                    and os.environ.get("AMDTRAIN_CONVSTEM", "custom")
                    == "custom"):
                # generic element-gather path (stem + odd shapes; full
                # fwd/dgrad/wgrad coverage)
                return conv_stem_mfma(x, self.weight, self.stride[0],
                                      self.padding[0])
        return super().forward(x)
