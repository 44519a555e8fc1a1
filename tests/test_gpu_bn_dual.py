"""Dual-BN block tail (downsample shortcut folded into the tail's kernels):
the fused path must reproduce the two-BN composition bit for bit — outputs,
every gradient and both BNs' running statistics — with and without a second
gradient operand arriving through the output's mailbox.  Also covers the
wide-C (fp32 C=2048) bitmask reduce against plain torch."""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _require_ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def _make_bn(C, seed):
    from amdtrain.models.resnet import FusedBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    bn = FusedBatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn.to(DEV).train()


def _run_tail(monkeypatch, fuse, go2, bn3_0, bnd_0, x3_0, xd_0, w1, w2):
    from amdtrain.ops import fused as OFU
    from amdtrain.ops.conv import ResidualGradTap
    monkeypatch.setenv("AMDTRAIN_DSFUSE", "1" if fuse else "0")
    bn3, bnd = copy.deepcopy(bn3_0), copy.deepcopy(bnd_0)
    x3 = x3_0.clone().requires_grad_(True)
    xd = xd_0.clone().requires_grad_(True)
    y = OFU.bn_add_relu_downsample(x3, bn3, xd, bnd)
    fn_name = type(y.grad_fn).__name__
    loss = (y.float() * w1).sum()
    if go2:
        # what the next residual block does: reroute its shortcut gradient
        # into this tail's backward through the published mailbox
        cell = y._amdtrain_next_cell
        cell.armed = True
        tapped = ResidualGradTap.apply(y, cell)
        loss = loss + (tapped.float() * w2).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = {"y": y.detach(), "gx3": x3.grad, "gxd": xd.grad}
    for tag, bn in (("3", bn3), ("d", bnd)):
        res["gw" + tag] = bn.weight.grad
        res["gb" + tag] = bn.bias.grad
        res["rm" + tag] = bn.running_mean
        res["rv" + tag] = bn.running_var
        res["nbt" + tag] = bn.num_batches_tracked
    return res, fn_name


# (N, C, HW, dtype, dual kernels expected)
#  * R=98 rows: odd tail for the 2-way unroll, uneven row split
#  * bf16 C=2048: C/VEC = 256, the register-path boundary
#  * fp32 C=2048: wide-C, must match through the fallback
_SHAPES = [
    (2, 64, 7, torch.bfloat16, True),
    (2, 64, 7, torch.float32, True),
    (1, 2048, 3, torch.bfloat16, True),
    (1, 2048, 3, torch.float32, False),
]


@pytest.mark.parametrize("go2", [False, True])
@pytest.mark.parametrize("N,C,HW,dtype,dual", _SHAPES)
def test_dual_tail_matches_unfused(monkeypatch, N, C, HW, dtype, dual, go2):
    _require_ext()
    torch.manual_seed(11)
    bn3, bnd = _make_bn(C, 1), _make_bn(C, 2)
    x3 = _nhwc(torch.randn(N, C, HW, HW, device=DEV).to(dtype))
    xd = _nhwc((torch.randn(N, C, HW, HW, device=DEV) * 1.5 + 0.2).to(dtype))
    w1 = _nhwc(torch.randn(N, C, HW, HW, device=DEV))
    w2 = _nhwc(torch.randn(N, C, HW, HW, device=DEV))
    fused, fname = _run_tail(monkeypatch, True, go2, bn3, bnd, x3, xd, w1, w2)
    plain, pname = _run_tail(monkeypatch, False, go2, bn3, bnd, x3, xd, w1,
                             w2)
    # the comparison must not be vacuous
    assert ("_BNDualFunction" in fname) == dual, fname
    assert "_BNDualFunction" not in pname, pname
    assert int(fused["nbt3"]) == 1 and int(fused["nbtd"]) == 1
    assert (fused["y"] > 0).any() and (fused["y"] == 0).any()
    for k in plain:
        assert fused[k].dtype == plain[k].dtype, k
        assert torch.equal(fused[k], plain[k]), (
            k, (fused[k].float() - plain[k].float()).abs().max().item())


def test_wide_c_bitmask_reduce_fp32():
    """fp32 C=2048 block tail: C/VEC = 512 takes the reduce kernel's wide-C
    branch, which must honour the forward ReLU bitmask (it used to compute
    unmasked gradients).  Tolerances are test_bn_add_relu_backward's fp32
    ones; the loss is linear in y so the incoming gradient is non-zero
    where the ReLU clamped (a sum of squares hides a missing mask)."""
    from amdtrain.models.resnet import FusedBatchNorm2d
    from amdtrain.ops import fused as OFU
    _require_ext()
    torch.manual_seed(3)
    C = 2048
    bn = FusedBatchNorm2d(C).to(DEV)
    ref = torch.nn.BatchNorm2d(C).to(DEV)
    ref.load_state_dict(bn.state_dict())

    x = torch.randn(2, C, 4, 4, device=DEV)
    z = torch.randn_like(x)
    w = torch.randn_like(x)
    xg = _nhwc(x).requires_grad_(True)
    zg = _nhwc(z).requires_grad_(True)
    y = OFU.bn_add_relu(xg, bn, zg)
    (y.float() * w).sum().backward()

    xr = x.detach().float().requires_grad_(True)
    zr = z.detach().float().requires_grad_(True)
    yr = F.relu(ref(xr) + zr)
    (yr * w).sum().backward()
    assert (yr == 0).any()

    tol, rtol = 2e-3, 1e-3
    assert torch.allclose(y.float(), yr, atol=tol, rtol=rtol)
    assert torch.allclose(xg.grad.float(), xr.grad, atol=tol * 5, rtol=rtol)
    assert torch.allclose(zg.grad.float(), zr.grad, atol=tol * 5, rtol=rtol)
    assert torch.allclose(bn.weight.grad, ref.weight.grad, atol=tol * 10,
                          rtol=rtol)
    assert torch.allclose(bn.bias.grad, ref.bias.grad, atol=tol * 10,
                          rtol=rtol)
