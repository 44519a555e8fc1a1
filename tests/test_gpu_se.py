"""Squeeze-excite and hardswish kernels (se.hip) against fp64 references,
their autograd wrappers, and mobilenet_v3_large on them.

Bounds (derived, not tuned).  u = 2^-24 is fp32's unit roundoff.  A result
that is a chain of fp32 sums with L terms in all satisfies, in any summation
order, |out - ref| <= (L - 1) u A to first order, where A is the same
quantity computed from absolute values (|a(x)|, |dy|, |W|, |b|, with the
ReLU and gate masks of the true forward pass kept as they are).  Every
other rounding on the way (the hardswish, 1/HW, the gate, products that do
not contract to an fma, the last two or three operations) adds at most u A;
there are fewer than 16 of them on any chain, so

    B(L, A) = 1.001 (L + 16) 2^-24 A        (1.001: the second-order terms)

  s:            B(HW + C + Cs, A)    mean -> FC1 -> FC2
  dm:           B(HW + C + Cs, A)    ds -> W2^T -> W1^T
  dW1, db1:     B(N + 2 HW + C, A)   sum_n dz1 (ds -> W2^T) x mean (HW)
  dW2, db2:     B(N + 2 HW + C, A)   sum_n dz2 (ds: HW) x h (HW + C)
  y  (bf16):    2^-8 |ref| + 1.01 |a(x)| B_s
  dx (bf16):    2^-8 |ref| + 1.01 (|a'(x)| (|dy| B_s + B_dm)
                                   + E (|dy| A_s + A_dm))

(a sum over a product of two inexact factors: the chain lengths add.)  One
bf16 rounding is 2^-9 relative; 2^-8 and 1.01 leave room for its product
with the fp32 term.  E = 2^-23 (|x| / 3 + 1 / 2) is the absolute error of
hardswish's slope fma(x, fl(1/3), 1/2): one rounding of the constant, one of
the result, and next to x = -3/2 nothing of the slope is left to hide them
in (E = 0 without hardswish, whose value x (x + 3) / 6 has no such
cancellation: x + 3 is exact for a bf16 x).  A bound B(L, A) only catches a
dropped term while it is below A / L, that is L (L + 16) < 2^24, asserted
for every case.  The
operands keep every pre-activation at least 0.25 away from the kinks of the
ReLU (at 0) and of the gate (at -3 and 3), so the masks of kernel and
reference agree; hardswish's own kinks are hit exactly, on purpose.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENV = "AMDTRAIN_SE"

# (N, C, H, W, Cs), forced splits (0: the host chooses)
CASES = [
    ((1, 8, 1, 1, 8), 0),        # one pack; the mean is the value
    ((2, 72, 7, 5, 24), 0),      # 9 packs; HW no multiple of the row slots
    ((3, 120, 14, 14, 32), 0),
    ((2, 960, 7, 7, 240), 0),    # the widest; Cs no multiple of a wave
    ((2, 2056, 3, 2, 520), 0),   # 257 packs
    ((1, 16, 40, 40, 8), 1),
    ((1, 16, 40, 40, 8), 3),
]
NAMES = ("s", "y", "dx", "dw1", "db1", "dw2", "db2")


def _B(L, A):
    assert L * (L + 16) < 2 ** 24
    return 1.001 * (L + 16) * 2.0 ** -24 * A


@functools.lru_cache(maxsize=None)
def _case(shape, pre_act):
    """Seeded operands, fp64 CPU references and bounds, shared read-only."""
    n, c, h, w, cs = shape
    hw, hs = h * w, pre_act == "hardswish"
    g = torch.Generator().manual_seed(c + 7 * hw + hs)
    x = (2.5 * torch.randn(n, c, h, w, generator=g)).bfloat16()
    x.view(-1)[:4] = torch.tensor([3.0, -3.0, 3.0, -3.0]).bfloat16()
    dy = torch.randn(n, c, h, w, generator=g).bfloat16()
    xd = x.double().requires_grad_(True)
    a = F.hardswish(xd) if hs else xd
    da = torch.autograd.grad(a.sum(), xd, retain_graph=True)[0].abs()
    mean = a.mean((2, 3))
    # |W1 mean| <= 0.25 around b1 = +-0.5 (a third of the units dead),
    # |W2 h| <= 0.5 around b2 = -4, 0, 4 (saturated low, linear, high)
    w1 = torch.randn(cs, c, generator=g).double()
    w1 = (w1 * 0.25 / (mean.detach() @ w1.t()).abs().max()).float()
    b1 = torch.where(torch.arange(cs) % 3 == 0, -0.5, 0.5).float()
    hid = F.relu(F.linear(mean.detach(), w1.double(), b1.double()))
    w2 = torch.randn(c, cs, generator=g).double()
    w2 = (w2 * 0.5 / (hid @ w2.t()).abs().max()).float()
    b2 = (4.0 * (torch.arange(c) % 3 - 1)).float()

    p = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    z1 = F.linear(mean, p[0], p[1])
    z2 = F.linear(F.relu(z1), p[2], p[3])
    assert (z1.abs() > 0.24).all() and ((z2.abs() - 3).abs() > 0.24).all()
    s = F.hardsigmoid(z2)
    y = a * s[:, :, None, None]
    ref = dict(zip(NAMES[2:], torch.autograd.grad(y, [xd] + p, dy.double())))
    ref.update(s=s.detach(), y=y.detach())

    # the same quantities from absolute values, true masks kept
    aA, dyA = a.detach().abs(), dy.double().abs()
    W1, W2 = w1.double().abs(), w2.double().abs()
    meanA = aA.mean((2, 3))
    hA = meanA @ W1.t() + b1.double().abs()
    sA = (hA @ W2.t() + b2.double().abs()) / 6 + 0.5
    dz2A = (dyA * aA).sum((2, 3)) / 6 * ((s > 0) & (s < 1))
    dz1A = (dz2A @ W2) * (z1 > 0)
    dmA = (dz1A @ W1) / hw
    Ls, Lw = hw + c + cs, n + 2 * hw + c
    Bs = _B(Ls, sA)
    E = 2.0 ** -23 * (x.double().abs() / 3 + 0.5) if hs else 0.0
    bound = dict(
        s=Bs,
        y=2.0 ** -8 * ref["y"].abs() + 1.01 * aA * Bs[:, :, None, None],
        dx=2.0 ** -8 * ref["dx"].abs() + 1.01 * (
            da * (dyA * Bs[:, :, None, None]
                  + _B(Ls, dmA)[:, :, None, None])
            + E * (dyA * sA[:, :, None, None] + dmA[:, :, None, None])),
        dw1=_B(Lw, dz1A.t() @ meanA), db1=_B(Lw, dz1A.sum(0)),
        dw2=_B(Lw, dz2A.t() @ hA), db2=_B(Lw, dz2A.sum(0)))
    return dict(x=x, dy=dy, w=(w1, b1, w2, b2), ref=ref, bound=bound)


def _rows_gpu(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous().to(DEV)


def _run_kernels(shape, pre_act, splits=0):
    from amdtrain import _C
    n, c, h, w, cs = shape
    hw, hs = h * w, pre_act == "hardswish"
    k = _case(shape, pre_act)
    x2d, dy2d = _rows_gpu(k["x"]), _rows_gpu(k["dy"])
    w1, b1, w2, b2 = (t.to(DEV) for t in k["w"])
    part = _C.se_squeeze(x2d, n, hw, hs, splits)
    s, mean, hid = _C.se_excite(part, hw, w1, b1, w2, b2)
    y2d = _C.se_scale(x2d, s, n, hw, hs)
    ds_part = _C.se_bwd_reduce(dy2d, x2d, n, hw, hs, splits)
    dz2, dz1, dm = _C.se_excite_bwd(ds_part, s, hid, w1, w2, hw)
    dw1, db1, dw2, db2 = _C.se_wgrad(dz2, dz1, mean, hid)
    dx2d = _C.se_bwd_apply(dy2d, x2d, s, dm, n, hw, hs)
    torch.cuda.synchronize()
    return dict(s=s, y=y2d, dx=dx2d, dw1=dw1, db1=db1, dw2=dw2, db2=db2,
                part=part, ds_part=ds_part)


def _check(name, out, ref, bound):
    err = (out - ref).abs()
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max (err - bound) {worst:.3e}")
    assert torch.isfinite(out).all(), name
    assert (err <= bound).all(), \
        f"{name}: {(err > bound).sum().item()} elements over the bound, " \
        f"worst excess {worst:.3e}"


@pytest.mark.parametrize("pre_act", ["none", "hardswish"])
@pytest.mark.parametrize("shape,splits", CASES)
def test_kernels_vs_fp64(shape, splits, pre_act):
    n, c, h, w, cs = shape
    k = _case(shape, pre_act)
    out = _run_kernels(shape, pre_act, splits)
    for name in ("part", "ds_part"):
        assert out[name].dtype == torch.float32 and out[name].dim() == 3
        assert out[name].shape[0] == n and out[name].shape[2] == c
        assert out[name].shape[1] == splits or (not splits
                                                and out[name].shape[1] >= 1)
    for name in ("y", "dx"):
        assert out[name].dtype == torch.bfloat16
        out[name] = out[name].view(n, h, w, c).permute(0, 3, 1, 2)
    for name in NAMES:
        assert out[name].shape == k["ref"][name].shape, name
        _check(name, out[name].double().cpu(), k["ref"][name],
               k["bound"][name])


@pytest.mark.parametrize("pre_act", ["none", "hardswish"])
def test_autograd_wrapper_matches_kernels(monkeypatch, pre_act):
    """squeeze_excite() on the GPU is the seven kernels: same bits, weight
    gradients in the shapes of the weights; a second run of the kernels gives
    the same bits."""
    from amdtrain.ops import squeeze_excite
    monkeypatch.delenv(ENV, raising=False)
    shape = (3, 120, 14, 14, 32)
    n, c, h, w, cs = shape
    k = _case(shape, pre_act)
    out, again = _run_kernels(shape, pre_act), _run_kernels(shape, pre_act)
    for name in NAMES:
        assert torch.equal(out[name], again[name]), name
    x = k["x"].to(DEV).contiguous(memory_format=torch.channels_last) \
        .requires_grad_(True)
    w1, b1, w2, b2 = (t.to(DEV).requires_grad_(True) for t in k["w"])
    w1c = w1.detach().view(cs, c, 1, 1).requires_grad_(True)
    y = squeeze_excite(x, w1c, b1, w2, b2, pre_act)
    assert y.dtype == torch.bfloat16 and y.shape == (n, c, h, w)
    y.backward(k["dy"].to(DEV))
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(-1, c), out["y"])
    assert torch.equal(x.grad.permute(0, 2, 3, 1).reshape(-1, c), out["dx"])
    assert tuple(w1c.grad.shape) == (cs, c, 1, 1)
    for t, name in ((w1c.grad.view(cs, c), "dw1"), (b1.grad, "db1"),
                    (w2.grad, "dw2"), (b2.grad, "db2")):
        assert torch.equal(t, out[name]), name


def test_hardswish_vs_fp64():
    """Flat kernels on 125 packs and a scalar tail of 3, kinks included."""
    from amdtrain.ops import hardswish
    g = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(1003, generator=g)).bfloat16()
    x[[0, 1, 1001, 1002]] = torch.tensor([3.0, -3.0, -3.0, 3.0]).bfloat16()
    dy = torch.randn(1003, generator=g).bfloat16()
    xd = x.double().requires_grad_(True)
    ref = F.hardswish(xd)
    (dref,) = torch.autograd.grad(ref, xd, dy.double())
    xg = x.to(DEV).requires_grad_(True)
    y = hardswish(xg)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and xg.grad.dtype == torch.bfloat16
    # one bf16 rounding of a value with a few fp32 roundings in it; the
    # slope's absolute error E of the module docstring
    _check("y", y.detach().double().cpu(), ref.detach(),
           2.0 ** -8 * ref.detach().abs())
    E = 2.0 ** -23 * (x.double().abs() / 3 + 0.5)
    _check("dx", xg.grad.double().cpu(), dref,
           2.0 ** -8 * dref.abs() + 1.01 * E * dy.double().abs())


def test_host_rejects_out_of_contract():
    from amdtrain import _C
    x12 = torch.zeros(2 * 4, 12, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(2 * 4, 16, device=DEV, dtype=torch.bfloat16)
    part = torch.zeros(2, 1, 16, device=DEV)
    f = lambda *shape: torch.zeros(*shape, device=DEV)  # noqa: E731
    for bad in [
        lambda: _C.se_squeeze(x12, 2, 4, False, 0),          # C = 12
        lambda: _C.se_squeeze(x, 2, 5, False, 0),            # rows != N*HW
        lambda: _C.se_squeeze(x.float(), 2, 4, False, 0),    # dtype
        lambda: _C.se_scale(x.float(), f(2, 16), 2, 4, True),
        lambda: _C.se_excite(part, 4, f(0, 16), f(0), f(16, 0), f(16)),
    ]:
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


def _count(monkeypatch):
    import amdtrain.ops.conv as conv
    import amdtrain.ops.se as se
    calls = {"se": 0, 3: 0, 5: 0}

    def counted_se(*args, real=se._se_kernels):
        calls["se"] += 1
        return real(*args)
    monkeypatch.setattr(se, "_se_kernels", counted_se)
    for k, name in ((3, "dwconv3x3"), (5, "dwconv5x5")):
        def counted(x, weight, stride=1, k=k, real=getattr(conv, name)):
            calls[k] += 1
            return real(x, weight, stride)
        monkeypatch.setattr(conv, name, counted)
    for name in (ENV, "AMDTRAIN_DWCONV", "AMDTRAIN_DWCONV5X5"):
        monkeypatch.delenv(name, raising=False)
    return calls


def test_empty_batch(monkeypatch):
    """N == 0 is served on the host: empty y and dx, zero weight gradients."""
    from amdtrain.ops import SqueezeExcite
    calls = _count(monkeypatch)
    se = SqueezeExcite(16, 8, "hardswish").to(DEV)
    x = torch.zeros(0, 16, 5, 7, device=DEV, dtype=torch.bfloat16) \
        .requires_grad_(True)
    y = se(x)
    assert calls["se"] == 1
    assert tuple(y.shape) == (0, 16, 5, 7) and y.dtype == torch.bfloat16
    y.backward(torch.zeros_like(y))
    torch.cuda.synchronize()
    assert tuple(x.grad.shape) == (0, 16, 5, 7)
    for p in se.parameters():
        assert p.grad.shape == p.shape and (p.grad == 0).all()


@pytest.mark.parametrize("env,n_se", [({}, 8), ({ENV: "0"}, 0)])
def test_dispatch_mobilenet_v3_large(monkeypatch, env, n_se):
    from amdtrain.models import build_model
    calls = _count(monkeypatch)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    torch.manual_seed(0)
    m = build_model("mobilenet_v3_large", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert calls == {"se": n_se, 3: 9, 5: 6}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_model_step(monkeypatch):
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD

    monkeypatch.delenv(ENV, raising=False)
    torch.manual_seed(0)
    m = build_model("mobilenet_v3_large").to(DEV) \
        .to(memory_format=torch.channels_last).train()
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    crit = CrossEntropyLoss()
    x_cpu = torch.randn(8, 3, 96, 96)
    t_cpu = torch.randint(0, 1000, (8,))
    x = x_cpu.to(DEV).contiguous(memory_format=torch.channels_last)
    t = t_cpu.to(DEV)
    for _ in range(2):
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(m(x), t)
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        for name, p in m.named_parameters():
            assert p.grad is not None, name
            assert torch.isfinite(p.grad).all(), name
        opt.step()
    torch.cuda.synchronize()

    # fp32 CPU twin of the weights as they stand, dropout off on both sides
    m.classifier[2].p = 0.0
    ref = build_model("mobilenet_v3_large")
    ref.load_state_dict({k: v.detach().cpu() for k, v in
                         m.state_dict().items()})
    ref.train()
    ref.classifier[2].p = 0.0
    out_ref = ref(x_cpu)
    F.cross_entropy(out_ref, t_cpu).backward()
    g_ref = ref.classifier[3].weight.grad

    def gpu_pass():
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
            loss = crit(out, t)
        loss.backward()
        torch.cuda.synchronize()
        return (_rel(out.detach().float().cpu(), out_ref.detach()),
                _rel(m.classifier[3].weight.grad.float().cpu(), g_ref))

    e_custom = gpu_pass()
    monkeypatch.setenv(ENV, "0")
    e_torch = gpu_pass()
    print(f"(logits, classifier.3.weight.grad): e_custom {e_custom} "
          f"e_torch {e_torch}")
    assert e_custom[0] <= 2 * e_torch[0] and e_custom[1] <= 2 * e_torch[1]
