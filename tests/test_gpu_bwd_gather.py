"""Backward operands gathered inside the BN kernels instead of materialized:
the stem pool gradient (AMDTRAIN_POOLBWD_FUSE), the pool output's second
gradient through the mailbox, the compact stride-2 shortcut gradient
(AMDTRAIN_DSGRAD_COMPACT), and the single-BN applies' coefficients in
registers (AMDTRAIN_BN_REGCOEF).  Every fused result must equal the
unfused one bit for bit, the sign of zero included."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCHES = ("AMDTRAIN_POOLBWD_FUSE", "AMDTRAIN_DSGRAD_COMPACT",
            "AMDTRAIN_BN_REGCOEF")


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def _bits(t):
    """Integer view, so +0.0 and -0.0 compare unequal."""
    t = t.detach().contiguous()
    if not t.is_floating_point():
        return t
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), (
        what, (a.float() - b.float()).abs().max().item())


def _ext():
    from amdtrain.ops import functional as OF
    from amdtrain.ops._ext import require_ext
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")
    return require_ext()


def _spy(monkeypatch, name):
    """Count calls of one extension entry point."""
    e = _ext()
    calls = []
    orig = getattr(e, name)

    def wrapped(*a, **k):
        calls.append(name)
        return orig(*a, **k)

    monkeypatch.setattr(e, name, wrapped)
    return calls


# ---- A: stem pool gradient gathered in the BN backward ----------------------

def _run_stem(monkeypatch, fuse, bn0, x0, w):
    from amdtrain.ops import fused as OFU
    monkeypatch.setenv("AMDTRAIN_POOLBWD_FUSE", "1" if fuse else "0")
    bn = copy.deepcopy(bn0)
    x = x0.clone().requires_grad_(True)
    y = OFU.bn_relu_max_pool(x, bn)
    assert "_BNReLUMaxPool" in type(y.grad_fn).__name__
    assert hasattr(y, "_amdtrain_next_cell") == fuse
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach(), "gx": x.grad, "gw": bn.weight.grad,
            "gb": bn.bias.grad}


# (2,64,14,14): plain even case; (3,16,13,11): odd sizes — edge windows and
# Ho = (H-1)/2+1; (2,64,10,10): R = 200 rows is no multiple of the reduce's
# row step (256 / (C/VEC) = 32)
@pytest.mark.parametrize("dtype,shape", [
    (torch.bfloat16, (2, 64, 14, 14)),
    (torch.bfloat16, (3, 16, 13, 11)),
    (torch.bfloat16, (2, 64, 10, 10)),
    (torch.float32, (3, 16, 13, 11)),
])
def test_stem_pool_gather_matches_unfused(monkeypatch, dtype, shape):
    from amdtrain.models.resnet import FusedBatchNorm2d
    _ext()
    torch.manual_seed(11)
    N, C, H, W = shape
    bn = FusedBatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.3)
        bn.bias[::8] = -10.0  # all-zero windows: the tie rule alone decides
    bn = bn.to(DEV).train()
    # integer-valued activations: many exact ties inside every window, so
    # the argmax codes decide which tap receives the gradient
    x = _nhwc(torch.randint(-3, 4, shape, device=DEV).to(dtype))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = _nhwc(torch.randn(N, C, Ho, Wo, device=DEV))
    pool_bwd = _spy(monkeypatch, "max_pool_3x3_s2_bwd")
    fused = _run_stem(monkeypatch, True, bn, x, w)
    assert not pool_bwd, "fused path still ran the pool backward kernel"
    plain = _run_stem(monkeypatch, False, bn, x, w)
    assert len(pool_bwd) == 1
    assert (fused["gx"] != 0).any()
    for k in plain:
        _assert_same(fused[k], plain[k], k)


# ---- B: the pool output's two consumers -------------------------------------

class _StemBlock(torch.nn.Module):
    """Stem + one Bottleneck with a stride-1 downsample (layer1 block 0)."""

    def __init__(self):
        super().__init__()
        from amdtrain.models import resnet as R
        self.conv1 = R.AmdConv2d(3, 64, kernel_size=7, stride=2, padding=3,
                                 bias=False)
        self.bn1 = R.FusedBatchNorm2d(64)
        down = torch.nn.Sequential(R.conv1x1(64, 256),
                                   R.FusedBatchNorm2d(256))
        self.block = R.Bottleneck(64, 64, 1, down)

    def forward(self, x):
        from amdtrain.ops import fused as OFU
        p = OFU.bn_relu_max_pool(self.conv1(x), self.bn1)
        self.cell = getattr(p, "_amdtrain_next_cell", None)
        return self.block(p)


def _run_module(model0, x0, w, autocast=True):
    model = copy.deepcopy(model0).train()
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = model(x)
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    out = {"y": y.detach(), "gx": x.grad}
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        out["grad:" + name] = p.grad
    for name, b in model.named_buffers():
        out["buf:" + name] = b
    return out, model


def test_pool_output_two_consumers(monkeypatch):
    _ext()
    torch.manual_seed(3)
    model = _StemBlock().to(DEV).to(memory_format=torch.channels_last)
    x = _nhwc(torch.randn(2, 3, 32, 32, device=DEV))
    w = _nhwc(torch.randn(2, 256, 8, 8, device=DEV))
    monkeypatch.setenv("AMDTRAIN_POOLBWD_FUSE", "1")
    fused, mf = _run_module(model, x, w)
    assert mf.cell is not None and mf.cell.armed and mf.cell.g is None
    monkeypatch.setenv("AMDTRAIN_POOLBWD_FUSE", "0")
    plain, mp = _run_module(model, x, w)
    assert mp.cell is None
    assert (fused["gx"] != 0).any()
    for k in plain:
        _assert_same(fused[k], plain[k], k)


# ---- C: compact stride-2 shortcut gradient ----------------------------------

@pytest.mark.parametrize("HW", [(8, 8), (7, 9)])
@pytest.mark.parametrize("C", [64, 256])
def test_compact_go2_kernel(C, HW):
    e = _ext()
    torch.manual_seed(C + HW[0])
    N, (H, W) = 2, HW
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    dt = torch.bfloat16
    x = _nhwc(torch.randn(N, C, H, W, device=DEV).to(dt))
    z = _nhwc(torch.randn(N, C, H, W, device=DEV).to(dt))
    weight = torch.rand(C, device=DEV) + 0.5
    bias = torch.randn(C, device=DEV) * 0.1
    rm = torch.zeros(C, device=DEV)
    rv = torch.ones(C, device=DEV)
    y, mean, invstd, scale, shift, mask = e.batch_norm_fwd_train(
        x, weight, bias, rm, rv, 0.1, 1e-5, True, z)
    go = _nhwc(torch.randn(N, C, H, W, device=DEV).to(dt))
    # -0.0 in go: off the even grid the materialized go2 contributes +0.0,
    # so ghat is +0.0 there — the fused reduce must do the same add
    go[:, ::3] = -0.0
    compact = torch.randn(N * Hs * Ws, C, device=DEV).to(dt)
    compact[::5] = -0.0
    dense = e.scatter_rows_x2(compact, N, H, W, Hs, Ws)
    ref = e.batch_norm_bwd(x, go, y, weight, mean, invstd, True, True,
                           scale, shift, dense, mask)
    got = e.batch_norm_bwd(x, go, y, weight, mean, invstd, True, True,
                           scale, shift, compact, mask, True)
    torch.cuda.synchronize()
    neg0 = torch.tensor(-0.0, dtype=dt).view(torch.int16).item()
    assert (_bits(go) == neg0).any()
    for name, a, b in zip(("gx", "gw", "gb", "ghat"), got, ref):
        _assert_same(a, b, name)
    # also without a saved relu mask (masked from y) and without relu
    empty = torch.empty(0, dtype=torch.uint8, device=DEV)
    for relu in (True, False):
        ref = e.batch_norm_bwd(x, go, y, weight, mean, invstd, relu, True,
                               scale, shift, dense, empty)
        got = e.batch_norm_bwd(x, go, y, weight, mean, invstd, relu, True,
                               scale, shift, compact, empty, True)
        for name, a, b in zip(("gx", "gw", "gb", "ghat"), got, ref):
            _assert_same(a, b, (name, relu))


class _TwoBlocks(torch.nn.Module):
    """Identity-shortcut Bottleneck feeding one with a stride-2 downsample."""

    def __init__(self):
        super().__init__()
        from amdtrain.models import resnet as R
        down = torch.nn.Sequential(R.conv1x1(256, 512, 2),
                                   R.FusedBatchNorm2d(512))
        self.a = R.Bottleneck(256, 64)
        self.b = R.Bottleneck(256, 128, 2, down)

    def forward(self, x):
        return self.b(self.a(x))


@pytest.mark.parametrize("HW", [8, 7])
def test_compact_go2_module(monkeypatch, HW):
    _ext()
    torch.manual_seed(9)
    model = _TwoBlocks().to(DEV).to(memory_format=torch.channels_last)
    x = _nhwc(torch.randn(2, 256, HW, HW, device=DEV).to(torch.bfloat16))
    Ho = (HW + 1) // 2
    w = _nhwc(torch.randn(2, 512, Ho, Ho, device=DEV))
    scatter = _spy(monkeypatch, "scatter_rows_x2")
    monkeypatch.setenv("AMDTRAIN_DSGRAD_COMPACT", "1")
    fused, _ = _run_module(model, x, w)
    assert not scatter, "compact path still scattered the shortcut gradient"
    monkeypatch.setenv("AMDTRAIN_DSGRAD_COMPACT", "0")
    plain, _ = _run_module(model, x, w)
    assert len(scatter) == 1
    for k in plain:
        _assert_same(fused[k], plain[k], k)


# ---- D: single-BN apply coefficients in registers ---------------------------

def _run_bn(monkeypatch, regc, bn0, x0, z0, relu, w):
    from amdtrain.ops import fused as OFU
    monkeypatch.setenv("AMDTRAIN_BN_REGCOEF", "1" if regc else "0")
    bn = copy.deepcopy(bn0)
    x = x0.clone().requires_grad_(True)
    z = None if z0 is None else z0.clone().requires_grad_(True)
    y = OFU.batch_norm(x, bn, relu=relu, addend=z)
    (y.float() * w).sum().backward()
    torch.cuda.synchronize()
    out = {"y": y.detach(), "gx": x.grad, "gw": bn.weight.grad,
           "gb": bn.bias.grad, "rm": bn.running_mean, "rv": bn.running_var}
    if z is not None:
        out["gz"] = z.grad
    return out


def _bn_case(monkeypatch, dtype, shape, relu, addend):
    from amdtrain.models.resnet import FusedBatchNorm2d
    _ext()
    torch.manual_seed(shape[1] + 2 * relu + addend)
    C = shape[1]
    bn = FusedBatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C) + 0.5)
        bn.bias.copy_(torch.randn(C) * 0.3)
    bn = bn.to(DEV).train()
    x = _nhwc(torch.randn(shape, device=DEV).to(dtype))
    z = _nhwc(torch.randn(shape, device=DEV).to(dtype)) if addend else None
    w = _nhwc(torch.randn(shape, device=DEV))
    reg = _run_bn(monkeypatch, True, bn, x, z, relu, w)
    lds = _run_bn(monkeypatch, False, bn, x, z, relu, w)
    assert (reg["gx"] != 0).any()
    for k in lds:
        _assert_same(reg[k], lds[k], k)


# relu without addend is the affine-mask backward (MASK 2); R = 2*5*5 = 50
# rows exercises the tail and the clamped second stream
@pytest.mark.parametrize("relu,addend", [(False, False), (True, False),
                                         (True, True)])
@pytest.mark.parametrize("C", [8, 64, 512, 2048])
def test_bn_register_coefficients(monkeypatch, C, relu, addend):
    _bn_case(monkeypatch, torch.bfloat16, (2, C, 5, 5), relu, addend)


@pytest.mark.parametrize("relu,addend", [(True, False), (True, True)])
def test_bn_register_coefficients_long_loop(monkeypatch, relu, addend):
    # 10*128*128*8 packs > 2 * 2048 * 256: the grid-stride loop runs more
    # than once per thread
    _bn_case(monkeypatch, torch.bfloat16, (10, 64, 128, 128), relu, addend)


def test_bn_register_coefficients_wide_fp32(monkeypatch):
    # fp32 C=2048 is C/VEC = 512 > 256: both settings take the LDS path
    _bn_case(monkeypatch, torch.float32, (2, 2048, 5, 5), True, False)


# ---- whole model -------------------------------------------------------------

def _step(monkeypatch, on, model0, x, target):
    from amdtrain.ops import CrossEntropyLoss
    for s in SWITCHES:
        monkeypatch.setenv(s, "1" if on else "0")
    model = copy.deepcopy(model0).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x)
    loss = CrossEntropyLoss()(out, target)
    loss.backward()
    torch.cuda.synchronize()
    return model, out.detach(), loss.detach()


# Bottleneck [2,1,1,1]: layer2's block follows a plain tail (compact path),
# layer3/4's follow a downsample (dual) tail, which keeps the scatter
@pytest.mark.parametrize("block,layers,scatters",
                         [("Bottleneck", [2, 1, 1, 1], 2),
                          ("BasicBlock", [1, 1, 1, 1], None)])
def test_model_switches_on_equals_off(monkeypatch, block, layers, scatters):
    from amdtrain.models import resnet as R
    _ext()
    torch.manual_seed(7)
    model = R.ResNet(getattr(R, block), layers, num_classes=16).to(DEV) \
        .to(memory_format=torch.channels_last)
    x = _nhwc(torch.randn(2, 3, 64, 64, device=DEV).to(torch.bfloat16))
    target = torch.tensor([3, 11], device=DEV)
    scatter = _spy(monkeypatch, "scatter_rows_x2")
    pool_bwd = _spy(monkeypatch, "max_pool_3x3_s2_bwd")
    mf, of, lf = _step(monkeypatch, True, model, x, target)
    assert not pool_bwd
    if scatters is not None:
        assert len(scatter) == scatters
    del scatter[:]
    mp, op, lp = _step(monkeypatch, False, model, x, target)
    assert len(pool_bwd) == 1
    if scatters is not None:
        assert len(scatter) == 3
    assert torch.isfinite(lf).item()
    _assert_same(lf, lp, "loss")
    _assert_same(of, op, "logits")
    pf, pp = dict(mf.named_parameters()), dict(mp.named_parameters())
    for name in pp:
        assert pf[name].grad is not None, name
        _assert_same(pf[name].grad, pp[name].grad, name)
    bf, bp = dict(mf.named_buffers()), dict(mp.named_buffers())
    for name in bp:
        assert torch.equal(bf[name], bp[name]), name
