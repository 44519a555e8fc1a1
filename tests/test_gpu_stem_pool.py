"""Stem BN+ReLU folded into the 3x3/s2 max pool's tap loop: output, argmax
routing (seen through the input gradient), parameter gradients and running
statistics must equal the BN-apply -> pool composition bit for bit."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def _run_stem(monkeypatch, fuse, bn0, x0, w):
    from amdtrain.ops import fused as OFU
    monkeypatch.setenv("AMDTRAIN_STEMFUSE", "1" if fuse else "0")
    bn = copy.deepcopy(bn0)
    x = x0.clone().requires_grad_(True)
    y = OFU.bn_relu_max_pool(x, bn)
    fn_name = type(y.grad_fn).__name__
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach(), "gx": x.grad, "gw": bn.weight.grad,
            "gb": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var,
            "nbt": bn.num_batches_tracked}, fn_name


# 14x14: even extent; 15x15: odd extent, partial windows on every edge
@pytest.mark.parametrize("HW", [14, 15])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stem_pool_matches_unfused(monkeypatch, dtype, HW):
    from amdtrain.models.resnet import FusedBatchNorm2d
    from amdtrain.ops import functional as OF
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")
    torch.manual_seed(5)
    C = 64
    bn = FusedBatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.3)
        # whole channels below zero after BN: every window is all-zero
        # post-ReLU, so the argmax is decided by the tie rule alone
        bn.bias[::8] = -10.0
    bn = bn.to(DEV).train()
    x = _nhwc(torch.randn(2, C, HW, HW, device=DEV).to(dtype))
    Ho = (HW - 1) // 2 + 1
    w = _nhwc(torch.randn(2, C, Ho, Ho, device=DEV))
    fused, fname = _run_stem(monkeypatch, True, bn, x, w)
    plain, pname = _run_stem(monkeypatch, False, bn, x, w)
    assert "_BNReLUMaxPool" in fname, fname
    assert "_BNReLUMaxPool" not in pname, pname
    assert int(fused["nbt"]) == 1
    assert (fused["y"][:, ::8] == 0).all() and (fused["y"] > 0).any()
    for k in plain:
        assert fused[k].dtype == plain[k].dtype, k
        assert torch.equal(fused[k], plain[k]), (
            k, (fused[k].float() - plain[k].float()).abs().max().item())
