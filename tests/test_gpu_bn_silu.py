"""BN + SiLU (batchnorm_anyc.h), the SiLU / sigmoid squeeze-excite MLP
(se.hip) and efficientnet_b0 on them, against fp64 CPU references from the
same bf16-rounded operands.

BN bounds are those of test_gpu_bn_anyc.py (u = 2^-9, R = N*H*W) with SiLU's
Lipschitz constant 1.1 (max |silu'| = 1.0998) where the clamps have 1:
  y:  2u |ref| + 2u 1.1 S_y, S_y = |scale||x| + |shift|
  gx: 2u |ref| + 2u S_gx, S_gx = |A| 1.1|go| + |B||x| + |D|
  gw, gb, running stats: 4 R 2^-23 Sabs, with 1.1 |go| for |ghat| in Sabs.
1.1 |go| and not |ghat|: the slope is taken at an fp32 v, off by dv of a few
2^-24 S_y, and moves by |silu''| dv <= dv / 2 also where it vanishes
(v = -1.28) and |ghat| could pay for nothing; the kernel's own slope error,
(|v| + 6) 2^-24, is of that size.  Two channels carry an outlier x = 64
under weight +-16: rows with v > 90 and v < -90, where exp overflows and the
outputs must be finite, v and 0 to within the same bounds.

SE bounds are B(L, A) of test_gpu_se.py, A taken with |silu'| <= 1.1 and
sigmoid' <= 1/4 in place of the masks (a ReLU hidden layer keeps its true
mask).  The sigmoids cost (|z| + 3) roundings each, |z1| <= 0.75,
|z2| <= 2.5: still fewer than 16 on any chain.
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from test_gpu_se import _B, _check, _count, _rel, _rows_gpu

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOM, U = 1e-5, 0.1, 2.0 ** -9


def _pc(t):
    return t.view(1, -1, 1, 1)


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _bn_case(shape, training=True):
    """Seeded bf16 operands, fp64 reference and bounds (shared, read-only)."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(shape, generator=g).bfloat16()
    x[0, :2, 0, 0] = 64.0
    go = torch.randn(shape, generator=g).bfloat16()
    weight = torch.rand(c, generator=g) * 2 + 2
    weight[:2] = torch.tensor([16.0, -16.0])
    bias = torch.rand(c, generator=g) * 2 + 1
    rm0 = torch.randn(c, generator=g) * 0.5
    rv0 = torch.rand(c, generator=g) + 0.5
    xd, god, dims, R = x.double(), go.double(), (0, 2, 3), n * h * w
    mean, sq = xd.mean(dims), (xd * xd).mean(dims)
    var = sq - mean * mean
    if not training:
        mean, var = rm0.double(), rv0.double()
    invstd = (var + EPS).rsqrt()
    a = weight.double() * invstd
    shift = bias.double() - mean * a
    v = _pc(a) * xd + _pc(shift)
    sg = torch.sigmoid(v)
    y = v * sg
    ghat, gA = god * sg * (1 + v * (1 - sg)), 1.1 * god.abs()
    gb, gw = ghat.sum(dims), (ghat * (xd - _pc(mean)) * _pc(invstd)).sum(dims)
    b = -a * invstd * gw / R
    d = -a * gb / R - b * mean
    gx = _pc(a) * ghat + _pc(b) * xd + _pc(d)
    s_y = _pc(a.abs()) * xd.abs() + _pc(shift.abs())
    s_gx = _pc(a.abs()) * gA + _pc(b.abs()) * xd.abs() + _pc(d.abs())
    t, unb = 4 * R * 2.0 ** -23, R / (R - 1)
    ref = dict(y=y, gx=gx, gw=gw, gb=gb, rm=(1 - MOM) * rm0 + MOM * mean,
               rv=(1 - MOM) * rv0 + MOM * var * unb)
    bound = dict(
        y=2 * U * y.abs() + 2 * U * 1.1 * s_y,
        gx=2 * U * gx.abs() + 2 * U * s_gx, gb=t * gA.sum(dims),
        gw=t * (gA * (xd.abs() + _pc(mean.abs())) * _pc(invstd)).sum(dims),
        rm=t * ((1 - MOM) * rm0.abs() + MOM * xd.abs().mean(dims)),
        rv=t * ((1 - MOM) * rv0 + MOM * (sq + mean * mean) * unb))
    return dict(x=x, go=go, p=(weight, bias, rm0, rv0), v=v, ref=ref,
                bound=bound)


def _make_bn(k):
    from amdtrain.models.resnet import FusedBatchNorm2d
    bn = FusedBatchNorm2d(k["x"].size(1), eps=EPS, momentum=MOM)
    with torch.no_grad():
        for dst, src in zip((bn.weight, bn.bias, bn.running_mean,
                             bn.running_var), k["p"]):
            dst.copy_(src)
    return bn.to(DEV)


# C = 32: a power of two on the any-C kernels, gpr 4; 144: block 252; 1152:
# gpr 144, one phase per block.  R = 50 is one row per reduce block; R = 4608
# is three, the least with a two-row step and then a one-row has2 tail, and
# its 663552 packs run the apply's grid-stride loop twice, tail included.
@pytest.mark.parametrize("shape", [(2, 32, 5, 5), (2, 144, 5, 5),
                                   (2, 1152, 5, 5), (2, 1152, 48, 48)])
def test_bn_silu_vs_fp64(monkeypatch, shape):
    from amdtrain.ops import fused
    monkeypatch.delenv("AMDTRAIN_BN_SILU", raising=False)
    monkeypatch.setattr(F, "silu", None)      # the kernels, or a TypeError
    k = _bn_case(shape)
    assert k["v"][0, 0, 0, 0] > 90 and k["v"][0, 1, 0, 0] < -90
    bn = _make_bn(k).train()
    x = _nhwc(k["x"]).requires_grad_(True)
    y = fused.batch_norm(x, bn, silu=True)
    y.backward(_nhwc(k["go"]))
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and bn.num_batches_tracked.item() == 1
    out = dict(y=y, gx=x.grad, gw=bn.weight.grad, gb=bn.bias.grad,
               rm=bn.running_mean, rv=bn.running_var)
    for name, o in out.items():
        _check(name, o.detach().double().cpu(), k["ref"][name],
               k["bound"][name])


def test_bn_silu_eval(monkeypatch):
    from amdtrain.ops import fused
    monkeypatch.setattr(F, "silu", None)
    k = _bn_case((2, 144, 5, 5), False)
    bn = _make_bn(k).eval()
    with torch.no_grad():
        y = fused.batch_norm(_nhwc(k["x"]), bn, silu=True)
    _check("y", y.double().cpu(), k["ref"]["y"], k["bound"]["y"])
    assert torch.equal(bn.running_var.cpu(), k["p"][3])


SE_NAMES = ("s", "y", "dx", "dw1", "db1", "dw2", "db2")


@functools.lru_cache(maxsize=None)
def _se_case(shape, hidden):
    n, c, h, w, cs = shape
    hw, silu = h * w, hidden == "silu"
    g = torch.Generator().manual_seed(c + 7 * hw + silu)
    x = (2.5 * torch.randn(n, c, h, w, generator=g)).bfloat16()
    dy = torch.randn(n, c, h, w, generator=g).bfloat16()
    xd = x.double().requires_grad_(True)
    mean = xd.mean((2, 3))
    hid_fn = F.silu if silu else F.relu
    # |W1 mean| <= 0.25 around b1 = +-0.5, |W2 h| <= 0.5 around b2 = -2, 0, 2
    w1 = torch.randn(cs, c, generator=g).double()
    w1 = (w1 * 0.25 / (mean.detach() @ w1.t()).abs().max()).float()
    b1 = torch.where(torch.arange(cs) % 3 == 0, -0.5, 0.5).float()
    hid = hid_fn(F.linear(mean.detach(), w1.double(), b1.double()))
    w2 = torch.randn(c, cs, generator=g).double()
    w2 = (w2 * 0.5 / (hid @ w2.t()).abs().max()).float()
    b2 = (2.0 * (torch.arange(c) % 3 - 1)).float()
    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    z1 = F.linear(mean, p[0], p[1])
    s = torch.sigmoid(F.linear(hid_fn(z1), p[2], p[3]))
    assert (z1.abs() > 0.24).all()          # a ReLU mask cannot flip
    y = xd * s[:, :, None, None]
    ref = dict(zip(SE_NAMES[2:],
                   torch.autograd.grad(y, [xd] + p, dy.double())))
    ref.update(s=s.detach(), y=y.detach())
    # the same quantities from absolute values
    xA, dyA = x.double().abs(), dy.double().abs()
    W1, W2 = w1.double().abs(), w2.double().abs()
    meanA = xA.mean((2, 3))
    hA = (meanA @ W1.t() + b1.double().abs()) * (1.1 if silu else 1.0)
    sA = (hA @ W2.t() + b2.double().abs()) / 4 + 0.5
    dz2A = (dyA * xA).sum((2, 3)) / 4
    dz1A = (dz2A @ W2) * (1.1 if silu else (z1 > 0))
    dmA = (dz1A @ W1) / hw
    Ls, Lw = hw + c + cs, n + 2 * hw + c
    Bs, Bdm = (_B(Ls, t)[:, :, None, None] for t in (sA, dmA))
    bound = dict(
        s=_B(Ls, sA), y=2.0 ** -8 * ref["y"].abs() + 1.01 * xA * Bs,
        dx=2.0 ** -8 * ref["dx"].abs() + 1.01 * (dyA * Bs + Bdm),
        dw1=_B(Lw, dz1A.t() @ meanA), db1=_B(Lw, dz1A.sum(0)),
        dw2=_B(Lw, dz2A.t() @ hA), db2=_B(Lw, dz2A.sum(0)))
    return dict(x=x, dy=dy, w=(w1, b1, w2, b2), ref=ref, bound=bound)


@pytest.mark.parametrize("shape,splits,hidden", [
    ((1, 8, 1, 1, 1), 0, "silu"), ((2, 144, 7, 5, 6), 0, "silu"),
    ((2, 1152, 7, 7, 48), 0, "silu"), ((1, 32, 40, 40, 8), 3, "silu"),
    ((2, 144, 7, 5, 6), 0, "relu")])
def test_se_mlp_vs_fp64(shape, splits, hidden):
    from amdtrain import _C
    n, c, h, w, cs = shape
    hw, hcode = h * w, int(hidden == "silu")
    k = _se_case(shape, hidden)
    x2d, dy2d = _rows_gpu(k["x"]), _rows_gpu(k["dy"])
    w1, b1, w2, b2 = (t.to(DEV) for t in k["w"])
    part = _C.se_squeeze(x2d, n, hw, False, splits)
    s, mean, hid, *z1 = _C.se_excite(part, hw, w1, b1, w2, b2, hcode, 1)
    assert len(z1) == hcode and part.shape[1] == (splits or part.shape[1])
    y2d = _C.se_scale(x2d, s, n, hw, False)
    ds_part = _C.se_bwd_reduce(dy2d, x2d, n, hw, False, splits)
    dz2, dz1, dm = _C.se_excite_bwd(ds_part, s, z1[0] if z1 else hid, w1, w2,
                                    hw, hcode, 1)
    dw1, db1, dw2, db2 = _C.se_wgrad(dz2, dz1, mean, hid)
    dx2d = _C.se_bwd_apply(dy2d, x2d, s, dm, n, hw, False)
    torch.cuda.synchronize()
    out = dict(s=s, y=y2d.view(n, h, w, c).permute(0, 3, 1, 2), dw1=dw1,
               dx=dx2d.view(n, h, w, c).permute(0, 3, 1, 2), db1=db1,
               dw2=dw2, db2=db2)
    for name in SE_NAMES:
        _check(name, out[name].double().cpu(), k["ref"][name],
               k["bound"][name])


def _b0(**kw):
    from amdtrain.models import build_model
    torch.manual_seed(0)
    return build_model("efficientnet_b0", **kw).to(DEV) \
        .to(memory_format=torch.channels_last).train()


@pytest.mark.parametrize("env,n_se", [("1", 16), ("0", 0)])
def test_dispatch_efficientnet_b0(monkeypatch, env, n_se):
    calls = _count(monkeypatch)
    monkeypatch.delenv("AMDTRAIN_BN_SILU", raising=False)
    monkeypatch.setenv("AMDTRAIN_SE", env)
    m = _b0(num_classes=10)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(_nhwc(torch.randn(2, 3, 64, 64)))
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert calls == {"se": n_se, 3: 7, 5: 9}


def test_model_step(monkeypatch):
    """Two FusedSGD steps, then one pass against an fp32 CPU twin: within
    twice the error of the same pass on the switches-off route."""
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    for name in ("AMDTRAIN_SE", "AMDTRAIN_BN_SILU"):
        monkeypatch.delenv(name, raising=False)
    m = _b0(stochastic_depth_prob=0.0)
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    crit = CrossEntropyLoss()
    x_cpu, t_cpu = torch.randn(8, 3, 96, 96), torch.randint(0, 1000, (8,))
    x, t = _nhwc(x_cpu), t_cpu.to(DEV)

    def gpu_pass():
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
            loss = crit(out, t)
        loss.backward()
        torch.cuda.synchronize()
        return out.detach().float().cpu(), loss

    for _ in range(2):
        assert torch.isfinite(gpu_pass()[1]).item()
        for name, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        opt.step()
    m.classifier[0].p = 0.0     # dropout off on both sides
    ref = build_model("efficientnet_b0", stochastic_depth_prob=0.0)
    ref.load_state_dict({k: v.detach().cpu()
                         for k, v in m.state_dict().items()})
    ref.train()
    ref.classifier[0].p = 0.0
    out_ref = ref(x_cpu)
    F.cross_entropy(out_ref, t_cpu).backward()

    def errors():
        out = gpu_pass()[0]
        return (_rel(out, out_ref.detach()),
                _rel(m.classifier[1].weight.grad.float().cpu(),
                     ref.classifier[1].weight.grad))
    e_custom = errors()
    monkeypatch.setenv("AMDTRAIN_SE", "0")
    monkeypatch.setenv("AMDTRAIN_BN_SILU", "0")
    e_torch = errors()
    print(f"(logits, classifier.1.weight.grad): e_custom {e_custom} "
          f"e_torch {e_torch}")
    assert e_custom[0] <= 2 * e_torch[0] and e_custom[1] <= 2 * e_torch[1]
