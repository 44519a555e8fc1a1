"""Model-level check of the downsample-tail and stem fusions: one training
step's loss, every parameter gradient and every buffer are identical with
AMDTRAIN_DSFUSE / AMDTRAIN_STEMFUSE on and off."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _step(monkeypatch, fuse, model0, x, target):
    from amdtrain.ops import CrossEntropyLoss
    monkeypatch.setenv("AMDTRAIN_DSFUSE", "1" if fuse else "0")
    monkeypatch.setenv("AMDTRAIN_STEMFUSE", "1" if fuse else "0")
    model = copy.deepcopy(model0).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x)
    loss = CrossEntropyLoss()(out, target)
    loss.backward()
    torch.cuda.synchronize()
    return model, out.detach(), loss.detach()


@pytest.mark.parametrize("block,layers", [("Bottleneck", [2, 1, 1, 1]),
                                          ("BasicBlock", [1, 1, 1, 1])])
def test_model_fused_equals_unfused(monkeypatch, block, layers):
    from amdtrain.models import resnet as R
    from amdtrain.ops import functional as OF
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")
    torch.manual_seed(7)
    model = R.ResNet(getattr(R, block), layers, num_classes=16).to(DEV) \
        .to(memory_format=torch.channels_last)
    x = torch.randn(2, 3, 64, 64, device=DEV).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    target = torch.tensor([3, 11], device=DEV)
    mf, of, lf = _step(monkeypatch, True, model, x, target)
    mp, op, lp = _step(monkeypatch, False, model, x, target)
    assert torch.isfinite(lf).item()
    assert torch.equal(lf, lp), (lf.item(), lp.item())
    assert torch.equal(of, op)
    pf, pp = dict(mf.named_parameters()), dict(mp.named_parameters())
    for name in pp:
        assert pf[name].grad is not None, name
        assert torch.equal(pf[name].grad, pp[name].grad), (
            name, (pf[name].grad - pp[name].grad).abs().max().item())
    bf, bp = dict(mf.named_buffers()), dict(mp.named_buffers())
    for name in bp:
        assert torch.equal(bf[name], bp[name]), name
