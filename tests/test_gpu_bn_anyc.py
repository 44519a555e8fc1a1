"""BatchNorm(+ReLU/ReLU6) kernels for any channel count (batchnorm_anyc.h)
against fp64 references, their dispatch through ops.fused.batch_norm, and the
mobilenet_v2 wiring.

Reference: fp64 on the CPU from the same dtype-rounded inputs.

Bounds (derived, not tuned).  u is the unit roundoff of the output dtype
(2^-9 bf16, 2^-24 fp32), R = N*H*W the rows a channel is reduced over.

  y, gx:  |o - ref| <= 2u |ref| + 2u S
          S is the fp64 sum of the absolute values of the terms that form
          ref: |scale||x| + |shift| (+ |z|) for y, |A||ghat| + |B||x| + |D|
          for gx.  The rounding of the output costs u |ref|; the fp32
          evaluation of the two or three terms, each at most S, and the
          fp32 coefficients cost a few 2^-24 S, far below u S in bf16.
          ReLU and ReLU6 clamp, which is 1-Lipschitz: the bound on y holds
          on both sides of a clamp boundary.
          In fp32 the coefficients are no longer exact at the scale of u:
          they come from mean, var, gw and gb, fp32 sums over R terms that
          by the rule below are off by up to t = 4 R 2^-23 of their
          absolute sums.  Carried through term by term, with
          k = max(1, (sum x^2/R + mean^2) / (var + eps)) the factor by
          which var's error relative to its absolute sum grows relative to
          var + eps (and so in invstd, scale and A):
            y:   dmean <= t mean|x| enters shift as scale dmean, the
                 relative error t k of scale enters scale (x - mean):
                 t k (|scale| (|x| + mean|x|) + |shift|)
            gx:  B = -A invstd gw/R and D = -A gb/R - B mean take gw's and
                 gb's errors t gw_abs, t gb_abs, and A's relative error:
                 t k (|A||ghat| + A invstd (gw_abs/R)(|x| + |mean|)
                      + A gb_abs/R)
          An fp32 output gets that term on top (t = 2.4e-5 at R = 50).  In
          bf16 it is below 1% of 2u S and is left out.
  gw, gb, running_mean, running_var:
          |o - ref| <= 4 R 2^-23 Sabs
          fp32 sums over R terms: any-order summation costs (R-1) 2^-24
          Sabs, doubled to R 2^-23 for the rounding of each term, times 4
          for the two-level fold (block partials, then collapse/finalize)
          and the handful of roundings of the final formula.  Sabs is the
          sum of the absolute terms: sum|ghat| for gb,
          sum|ghat|(|x| + |mean|) invstd for gw (xhat = (x - mean) invstd
          expanded), 0.9|rm0| + 0.1 sum|x|/R for running_mean and
          0.9|rv0| + 0.1 (sum x^2/R + mean^2) R/(R-1) for running_var.

An element whose pre-activation v lies within rounding of 0 or 6 may fall on
either side of the gradient mask.  The bounds are not loosened for that: the
loss is (y.float() * w).sum() with w zeroed on A = {|v| < 1e-3 or
|v - 6| < 1e-3} (1e-3 is > 50x the fp32 error of v here), so a flip changes
no gradient, |A| <= 1% of the elements is asserted, and so is that each clamp
holds >= 5% of them.  bn.weight ~ U(2,4), bn.bias ~ U(1,3), x ~ N(0,1) make
v roughly N(2, 3^2): ~25% below 0, ~9% above 6.

One case decides the mask from a v that differs from the reference's by more
than fp32 rounding, and gets a wider A by the same principle (still <= 1%,
asserted): with conv-epilogue partials the statistics are those of the
conv's unrounded fp32 output, the reference's those of its bf16 rounding.
Per element the two differ by at most u|x|, so mean moves by at most
u mean|x| and v by about |scale| u mean|x| ~ 3 * 2^-9 * 0.8 = 5e-3: both
margins are 1e-2 there.

Without the any-C kernels every test here fails: batch_norm has no relu6
keyword and sends every C that is no power of two to the library.

Not tested here: ReLU6 for a C outside the kernels' contract.  batch_norm
raises for it on the GPU (test_host_contract); the library composition
F.relu6(F.batch_norm(x)) that would serve it is not part of this op, see
TODO.md ("BN -> ReLU6 outside the any-C contract").
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
MOM = 0.1
UNIT = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11,
        torch.float32: 2.0 ** -24}

C_CASES = [24, 144, 160, 576, 960, 1280]   # gpr 3, 18, 20, 72, 120, 160
ACT_CASES = [("none", False), ("relu", False), ("relu6", False),
             ("none", True)]


def _pc(t):
    return t.view(1, -1, 1, 1)


def _reference(x, z, go, weight, bias, rm0, rv0, act, training=True,
               margin0=1e-3, margin6=1e-3):
    """fp64 BN(+z)(+act) forward and backward from dtype-rounded operands.
    ``go`` is zeroed on the boundary set A before the backward."""
    x, go = x.double(), go.double().clone()
    weight, bias = weight.double(), bias.double()
    rm0, rv0 = rm0.double(), rv0.double()
    c = x.size(1)
    R = x.numel() // c
    dims = (0, 2, 3)
    if training:
        mean = x.mean(dims)
        var = (x * x).mean(dims) - mean * mean
    else:
        mean, var = rm0, rv0
    invstd = (var + EPS).rsqrt()
    scale = weight * invstd
    shift = bias - mean * scale
    v = _pc(scale) * x + _pc(shift)
    s_y = _pc(scale.abs()) * x.abs() + _pc(shift.abs())
    if z is not None:
        v = v + z.double()
        s_y = s_y + z.double().abs()
    if act == "relu":
        y, passes = v.clamp(min=0), v > 0
        near = v.abs() < margin0
    elif act == "relu6":
        y, passes = v.clamp(0, 6), (v > 0) & (v < 6)
        near = (v.abs() < margin0) | ((v - 6).abs() < margin6)
    else:
        y, passes = v, torch.ones_like(v, dtype=torch.bool)
        near = torch.zeros_like(passes)
    go[near] = 0
    ghat = go * passes
    xhat = (x - _pc(mean)) * _pc(invstd)
    gb = ghat.sum(dims)
    gw = (ghat * xhat).sum(dims)
    a = weight * invstd
    b = -a * invstd * gw / R
    d = -a * gb / R - b * mean
    gx = _pc(a) * ghat + _pc(b) * x + _pc(d)
    s_gx = _pc(a.abs()) * ghat.abs() + _pc(b.abs()) * x.abs() + _pc(d.abs())
    unb = R / (R - 1) if R > 1 else 1.0
    gb_abs = ghat.abs().sum(dims)
    gw_abs = (ghat.abs() * (x.abs() + _pc(mean.abs()))
              * _pc(invstd)).sum(dims)
    # fp32 coefficient terms, see the docstring
    kap = (((x * x).mean(dims) + mean * mean) / (var + EPS)).clamp(min=1)
    c_y = _pc(kap) * (_pc(scale.abs()) * (x.abs() + _pc(x.abs().mean(dims)))
                      + _pc(shift.abs()))
    c_gx = _pc(kap) * (_pc(a.abs()) * ghat.abs()
                       + _pc(a.abs() * invstd * gw_abs / R)
                       * (x.abs() + _pc(mean.abs()))
                       + _pc(a.abs() * gb_abs / R))
    return dict(
        R=R, v=v, near=near, go=go, y=y, s_y=s_y, gx=gx, s_gx=s_gx,
        c_y=c_y, c_gx=c_gx,
        gz=ghat, gb=gb, gb_abs=gb_abs, gw=gw, gw_abs=gw_abs,
        rm=(1 - MOM) * rm0 + MOM * mean,
        rm_abs=(1 - MOM) * rm0.abs() + MOM * x.abs().mean(dims),
        rv=(1 - MOM) * rv0 + MOM * var * unb,
        rv_abs=(1 - MOM) * rv0.abs()
        + MOM * ((x * x).mean(dims) + mean * mean) * unb)


def _assert_shares(ref, act):
    """Both clamps really exercised, next to no element on a boundary."""
    n = ref["v"].numel()
    assert ref["near"].sum().item() <= 0.01 * n
    if act in ("relu", "relu6"):
        assert (ref["v"] < 0).sum().item() >= 0.05 * n
    if act == "relu6":
        assert (ref["v"] > 6).sum().item() >= 0.05 * n


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, act, with_add, training=True):
    """Seeded dtype-rounded operands and their fp64 reference; computed once
    per case and shared (read-only) by the tests."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(
        100000 * n + 10 * c + h + {"none": 1, "relu": 2, "relu6": 3}[act]
        + (7 if with_add else 0))
    x = torch.randn(shape, generator=g).to(dtype)
    z = torch.randn(shape, generator=g).to(dtype) if with_add else None
    go = torch.randn(shape, generator=g).to(dtype)
    weight = torch.rand(c, generator=g) * 2 + 2
    bias = torch.rand(c, generator=g) * 2 + 1
    rm0 = torch.randn(c, generator=g) * 0.5
    rv0 = torch.rand(c, generator=g) + 0.5
    ref = _reference(x, z, go, weight, bias, rm0, rv0, act, training)
    _assert_shares(ref, act)
    return dict(shape=shape, dtype=dtype, act=act, x=x, z=z, weight=weight,
                bias=bias, rm0=rm0, rv0=rv0, ref=ref)


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _make_bn(k):
    from amdtrain.models.resnet import FusedBatchNorm2d
    bn = FusedBatchNorm2d(k["shape"][1], eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.weight.copy_(k["weight"])
        bn.bias.copy_(k["bias"])
        bn.running_mean.copy_(k["rm0"])
        bn.running_var.copy_(k["rv0"])
    return bn.to(DEV)


def _run(k, backward=True):
    """One training forward (+ backward) through ops.fused.batch_norm."""
    from amdtrain.ops import fused
    act = k["act"]
    bn = _make_bn(k).train()
    x = _nhwc(k["x"]).requires_grad_(True)
    z = None if k["z"] is None else _nhwc(k["z"]).requires_grad_(True)
    y = fused.batch_norm(x, bn, relu=act == "relu", addend=z,
                         relu6=act == "relu6")
    out = dict(y=y.detach(), rm=bn.running_mean, rv=bn.running_var,
               nbt=bn.num_batches_tracked.item())
    if backward:
        # w: the reference's go, already zeroed on the boundary set, exactly
        # representable in y's dtype; NHWC like y, so that the gradient
        # arrives in the layout a model's would
        w = _nhwc(k["ref"]["go"].float())
        (y.float() * w).sum().backward()
        out.update(gx=x.grad, gw=bn.weight.grad, gb=bn.bias.grad,
                   gz=None if z is None else z.grad)
    torch.cuda.synchronize()
    return out


def _check(name, out, ref, bound):
    out = out.detach().double().cpu()
    err = (out - ref).abs()
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max (err - bound) {worst:.3e}, "
          f"max err/bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert out.shape == ref.shape, name
    assert torch.isfinite(out).all(), name
    assert (err <= bound).all(), \
        f"{name}: {(err > bound).sum().item()} elements over the bound, " \
        f"worst excess {worst:.3e}"


def _out_bound(ref, s, coef, dtype, R):
    u = UNIT[dtype]
    bound = 2 * u * ref.abs() + 2 * u * s
    if dtype == torch.float32:      # coefficient term, see the docstring
        bound = bound + 4 * R * 2.0 ** -23 * coef
    return bound


def _check_all(k, out, stats=True):
    ref, dtype = k["ref"], k["dtype"]
    R = ref["R"]
    assert out["y"].dtype == dtype and out["gx"].dtype == dtype
    _check("y", out["y"], ref["y"],
           _out_bound(ref["y"], ref["s_y"], ref["c_y"], dtype, R))
    _check("gx", out["gx"], ref["gx"],
           _out_bound(ref["gx"], ref["s_gx"], ref["c_gx"], dtype, R))
    if not stats:
        return
    sum_tol = 4 * R * 2.0 ** -23
    assert out["gw"].dtype == torch.float32
    _check("gw", out["gw"], ref["gw"], sum_tol * ref["gw_abs"])
    _check("gb", out["gb"], ref["gb"], sum_tol * ref["gb_abs"])
    _check("running_mean", out["rm"], ref["rm"], sum_tol * ref["rm_abs"])
    _check("running_var", out["rv"], ref["rv"], sum_tol * ref["rv_abs"])
    assert out["nbt"] == 1
    if k["z"] is not None:
        # no activation: the addend's gradient is grad_out itself
        assert torch.equal(out["gz"].double().cpu(), ref["gz"])


def _spy(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)

    monkeypatch.setattr(owner, name, counted)
    return calls


def _spy_library(monkeypatch):
    from amdtrain.ops import fused
    return (_spy(monkeypatch, fused, "_bn_torch"),
            _spy(monkeypatch, torch.nn.functional, "relu6"))


# 1. kernels against fp64: R = 50, ragged last phase, clamped second stream
@pytest.mark.parametrize("act,with_add", ACT_CASES)
@pytest.mark.parametrize("c", C_CASES)
def test_kernels_vs_fp64(monkeypatch, c, act, with_add):
    lib = _spy_library(monkeypatch)
    k = _case((2, c, 5, 5), torch.bfloat16, act, with_add)
    _check_all(k, _run(k))
    assert lib == ([], [])


# 2. fewer rows than phases: R = 4 < 85
def test_fewer_rows_than_phases(monkeypatch):
    k = _case((1, 24, 2, 2), torch.bfloat16, "relu6", False)
    _check_all(k, _run(k))


# 3. the grid-stride loops run more than once: 1.2 M packs > 2 x 2048 x 255
def test_grid_stride_more_than_once(monkeypatch):
    # not cached: the fp64 reference of 9.6 M elements is not worth keeping
    k = _case.__wrapped__((8, 24, 224, 224), torch.bfloat16, "relu6", False)
    assert k["x"].numel() // 8 > 2 * 2048 * 255
    _check_all(k, _run(k), stats=False)


# 4. fp32: gpr 6 on the kernels, gpr 320 outside the contract
def test_fp32(monkeypatch):
    lib = _spy_library(monkeypatch)
    k = _case((2, 24, 5, 5), torch.float32, "relu6", False)
    _check_all(k, _run(k))
    assert lib == ([], [])


def test_fp32_wide_falls_back(monkeypatch):
    """gpr 320 without an activation keeps the library BN, as before the
    any-C kernels; with ReLU6 there is no kernel and no composition."""
    from amdtrain.ops import fused
    bn_torch, _ = _spy_library(monkeypatch)
    k = _case((2, 1280, 5, 5), torch.float32, "none", False)
    out = _run(k)
    assert bn_torch == ["_bn_torch"]
    _check_all(k, out)
    bn = _make_bn(k).train()
    assert not fused.bn_relu6_fusable(_nhwc(k["x"]))
    with pytest.raises(NotImplementedError):
        fused.batch_norm(_nhwc(k["x"]), bn, relu6=True)
    assert bn.num_batches_tracked.item() == 0
    assert len(bn_torch) == 1


# 5. eval mode: running statistics, no reduce
def test_eval(monkeypatch):
    from amdtrain.ops import fused
    lib = _spy_library(monkeypatch)
    k = _case((2, 144, 5, 5), torch.bfloat16, "relu6", False, False)
    bn = _make_bn(k).eval()
    with torch.no_grad():
        y = fused.batch_norm(_nhwc(k["x"]), bn, relu6=True)
    torch.cuda.synchronize()
    ref = k["ref"]
    assert y.dtype == torch.bfloat16
    _check("y", y, ref["y"], _out_bound(ref["y"], ref["s_y"], ref["c_y"],
                                        torch.bfloat16, ref["R"]))
    assert torch.equal(bn.running_mean.cpu(), k["rm0"])
    assert torch.equal(bn.running_var.cpu(), k["rv0"])
    assert bn.num_batches_tracked.item() == 0
    assert lib == ([], [])


# 6. statistics from the 1x1 conv's epilogue partials
@pytest.mark.parametrize("fuse", ["1", "0"])
def test_stats_from_conv_partials(monkeypatch, fuse):
    """The reference is the fp64 BN of the conv's bf16 output, the tensor the
    apply reads.  With partials the statistics come from the conv's fp32
    accumulators, before that rounding: per element that moves x by at most
    u|x|, which is one of the two u S the bound grants."""
    from amdtrain import _C
    from amdtrain.ops import fused
    from amdtrain.ops.conv import AmdConv2d
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", fuse)
    lib = _spy_library(monkeypatch)
    from_parts = _spy(monkeypatch, _C, "batch_norm_fwd_train_from_parts")
    g = torch.Generator().manual_seed(192)
    conv = AmdConv2d(32, 192, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(192, 32, 1, 1, generator=g)
                           * 32 ** -0.5).bfloat16())
    conv = conv.to(DEV).to(torch.bfloat16)
    xin = torch.randn(2, 32, 6, 6, generator=g).bfloat16()
    go = torch.randn(2, 192, 6, 6, generator=g).bfloat16()
    weight = torch.rand(192, generator=g) * 2 + 2
    bias = torch.rand(192, generator=g) * 2 + 1
    rm0 = torch.zeros(192)
    rv0 = torch.ones(192)
    with torch.no_grad():
        xc = conv(_nhwc(xin))
    assert (getattr(xc, "_amdtrain_bn_stats", None) is not None) \
        == (fuse == "1")
    ref = _reference(xc.cpu(), None, go, weight, bias, rm0, rv0, "relu6",
                     margin0=1e-2, margin6=1e-2)
    _assert_shares(ref, "relu6")
    k = dict(shape=(2, 192, 6, 6), dtype=torch.bfloat16, act="relu6",
             x=None, z=None, weight=weight, bias=bias, rm0=rm0, rv0=rv0,
             ref=ref)
    bn = _make_bn(k).train()
    xc.requires_grad_(True)
    y = fused.batch_norm(xc, bn, relu6=True)
    (y.float() * _nhwc(ref["go"].float())).sum().backward()
    torch.cuda.synchronize()
    assert len(from_parts) == (1 if fuse == "1" else 0)
    assert lib == ([], [])
    _check_all(k, dict(y=y.detach(), gx=xc.grad), stats=False)


# 7. determinism: fixed reduction order, no atomics
def test_bitwise_deterministic(monkeypatch):
    k = _case((2, 144, 5, 5), torch.bfloat16, "relu6", False)
    a, b = _run(k), _run(k)
    for name in ("y", "gx", "gw", "gb", "rm", "rv"):
        assert torch.equal(a[name], b[name]), name


# 8. dispatch: nothing of mobilenet_v2's BN or ReLU6 leaves the kernels
def test_dispatch_mobilenet(monkeypatch):
    from amdtrain.models import build_model
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    bn_torch, relu6 = _spy_library(monkeypatch)

    def step():
        del bn_torch[:], relu6[:]
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        y.float().sum().backward()
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        for name, p in m.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
        return len(bn_torch), len(relu6)

    assert step() == (0, 0)


# 9. the routing guards, with the library BN stubbed out: without ReLU6, a C
# outside the kernels' contract and ReLU with an addend keep the library BN
# they always took; ReLU6 outside the contract raises.
def test_routing_outside_the_contract(monkeypatch):
    from amdtrain.ops import fused
    seen = []

    def stub(x, bn, relu, addend, relu6=False):
        seen.append((x.size(1), bool(relu), addend is not None, bool(relu6)))
        return x

    monkeypatch.setattr(fused, "_bn_torch", stub)
    k = _case((2, 24, 5, 5), torch.bfloat16, "none", True)
    bn = _make_bn(k).train()
    x = _nhwc(k["x"])
    x12 = _nhwc(torch.zeros(2, 12, 5, 5, dtype=torch.bfloat16))
    assert fused.bn_relu6_fusable(x) and not fused.bn_relu6_fusable(x12)
    assert fused.batch_norm(x12, bn) is x12
    # ReLU with an addend is the block tail: power-of-two C only
    assert fused.batch_norm(x, bn, relu=True, addend=x) is x
    assert seen == [(12, False, False, False), (24, True, True, False)]
    with pytest.raises(NotImplementedError):
        fused.batch_norm(x12, bn, relu6=True)
    assert len(seen) == 2
    assert bn.num_batches_tracked.item() == 2
    assert bn.running_mean.cpu().equal(k["rm0"])    # no kernel ran


# 10. host contract
def test_host_contract(monkeypatch):
    from amdtrain import _C
    from amdtrain.ops import fused
    k = _case((2, 24, 5, 5), torch.bfloat16, "none", True)
    bn = _make_bn(k).train()
    x, z = _nhwc(k["x"]), _nhwc(k["z"])
    with pytest.raises(ValueError):
        fused.batch_norm(x, bn, relu6=True, addend=z)
    with pytest.raises(ValueError):
        fused.batch_norm(x, bn, relu=True, relu6=True)
    assert bn.num_batches_tracked.item() == 0
    args = (x, bn.weight, bn.bias, bn.running_mean.clone(),
            bn.running_var.clone(), MOM, EPS)
    with pytest.raises(RuntimeError):       # the entry itself: relu6 + addend
        _C.batch_norm_fwd_train(*args, False, z, True)
    with pytest.raises(RuntimeError):       # relu and relu6
        _C.batch_norm_fwd_train(*args, True, None, True)
    with pytest.raises(RuntimeError):       # gpr 320 > 256
        _C.batch_norm_fwd_train(
            torch.zeros(1, 1280, 2, 2, device=DEV).contiguous(
                memory_format=torch.channels_last),
            torch.ones(1280, device=DEV), torch.zeros(1280, device=DEV),
            torch.zeros(1280, device=DEV), torch.ones(1280, device=DEV),
            MOM, EPS, False, None, True)
    y, mean, invstd, scale, shift, _ = _C.batch_norm_fwd_train(
        *args, False, None, True)
    with pytest.raises(RuntimeError):       # any-C backward with a grad_out2
        _C.batch_norm_bwd(x, z, y, bn.weight, mean, invstd, False, False,
                          scale, shift, z, None, False, True)
    torch.cuda.synchronize()
