"""Depthwise 5x5 halo-tile kernels (dwconv5x5.hip) against fp64 references,
their dispatch through AmdConv2d, and an mnasnet1_0 training step.

Bounds (derived, not tuned).  ``A`` is the reference quantity with every
operand replaced by its absolute value, i.e. the sum of the absolute terms.

  y, dx:  |out - ref| <= 2^-8 |ref| + 2^-19 A
          one bf16 rounding is at most 2^-9 relative; at most 25 fp32
          additions of exact bf16 products cost at most 25 * 2^-24 * A.
  dw:     |out - ref| <= L * 2^-23 * A,  L = N*Ho*Wo
          the any-order fp32 summation bound (L-1) * 2^-24 * A, doubled.
          It only catches a dropped term while L^2 < 2^23: L <= 2000 here.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"

SHAPES = [
    (1, 8, 1, 1),       # only the centre tap is inside
    (3, 40, 5, 3),      # narrower than a strip and than the halo, H != W
    (2, 72, 15, 15),    # odd size, stride 2 on odd size
    (2, 120, 14, 14),   # even size
    (1, 1152, 7, 7),    # widest layer
    (1, 2056, 3, 2),    # 257 packs
    (2, 144, 18, 34),   # 3 x 3 x 2 tiles (rows, columns, packs); s2: 2 x 2 x 2
]
CASES = [(s, st) for s in SHAPES for st in (1, 2)]
ENVS = ("AMDTRAIN_DWCONV", "AMDTRAIN_DWCONV5X5")


def _out_hw(h, w, stride):
    return (h + 4 - 5) // stride + 1, (w + 4 - 5) // stride + 1


@functools.lru_cache(maxsize=None)
def _case(shape, stride):
    """Seeded bf16 operands and fp64 CPU references, shared read-only."""
    n, c, h, w = shape
    ho, wo = _out_hw(h, w, stride)
    g = torch.Generator().manual_seed(1000 * c + 10 * h + stride)
    x = torch.randn(n, c, h, w, generator=g).bfloat16()
    dy = torch.randn(n, c, ho, wo, generator=g).bfloat16()
    wt = (torch.randn(c, 1, 5, 5, generator=g) / 5).bfloat16()

    def ref(xx, ww, gg):
        xx = xx.double().requires_grad_(True)
        ww = ww.double().requires_grad_(True)
        y = F.conv2d(xx, ww, None, stride, 2, 1, c)
        dx, dw = torch.autograd.grad(y, (xx, ww), gg.double())
        return y.detach(), dx, dw

    y, dx, dw = ref(x, wt, dy)
    ya, dxa, dwa = ref(x.abs(), wt.abs(), dy.abs())
    return dict(x=x, dy=dy, w=wt, y=y, dx=dx, dw=dw, ya=ya, dxa=dxa,
                dwa=dwa, ho=ho, wo=wo)


def _rows_gpu(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous().to(DEV)


def _nchw64(t2d, n, h, w, c):
    return t2d.view(n, h, w, c).permute(0, 3, 1, 2).double().cpu()


def _run_kernels(shape, stride):
    from amdtrain import _C
    n, c, h, w = shape
    k = _case(shape, stride)
    x2d, dy2d = _rows_gpu(k["x"]), _rows_gpu(k["dy"])
    w25 = k["w"].reshape(c, 25).t().contiguous().to(DEV)
    y2d = _C.dwconv5x5_fwd(x2d, n, h, w, stride, w25)
    dx2d = _C.dwconv5x5_dgrad(dy2d, n, h, w, stride, w25)
    dw25 = _C.dwconv5x5_wgrad(dy2d, x2d, n, h, w, stride)
    torch.cuda.synchronize()
    return y2d, dx2d, dw25


def _check(name, out, ref, bound):
    err = (out - ref).abs()
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max (err - bound) {worst:.3e}")
    assert torch.isfinite(out).all(), name
    assert (err <= bound).all(), \
        f"{name}: {(err > bound).sum().item()} elements over the bound, " \
        f"worst excess {worst:.3e}"


@pytest.mark.parametrize("shape,stride", CASES)
def test_kernels_vs_fp64(shape, stride):
    n, c, h, w = shape
    k = _case(shape, stride)
    ho, wo = k["ho"], k["wo"]
    y2d, dx2d, dw25 = _run_kernels(shape, stride)
    assert tuple(y2d.shape) == (n * ho * wo, c) and y2d.dtype == torch.bfloat16
    assert tuple(dx2d.shape) == (n * h * w, c) and dx2d.dtype == torch.bfloat16
    assert tuple(dw25.shape) == (25, c) and dw25.dtype == torch.float32

    y = _nchw64(y2d, n, ho, wo, c)
    dx = _nchw64(dx2d, n, h, w, c)
    dw = dw25.t().reshape(c, 1, 5, 5).double().cpu()
    L = n * ho * wo
    assert L <= 2000
    _check("y", y, k["y"], 2.0 ** -8 * k["y"].abs() + 2.0 ** -19 * k["ya"])
    _check("dx", dx, k["dx"],
           2.0 ** -8 * k["dx"].abs() + 2.0 ** -19 * k["dxa"])
    _check("dw", dw, k["dw"], L * 2.0 ** -23 * k["dwa"])


@pytest.mark.parametrize("stride", [1, 2])
def test_autograd_wrapper_matches_kernels(stride):
    """dwconv5x5() on the GPU is the three kernels: same bits, dw returned
    as [C, 1, 5, 5]; a second run of the kernels gives the same bits."""
    from amdtrain.ops.conv import dwconv5x5
    shape = (2, 72, 15, 15)
    n, c, h, w = shape
    k = _case(shape, stride)
    y2d, dx2d, dw25 = _run_kernels(shape, stride)
    for name, p, q in zip(("y", "dx", "dw"), (y2d, dx2d, dw25),
                          _run_kernels(shape, stride)):
        assert torch.equal(p, q), name
    x = k["x"].to(DEV).contiguous(memory_format=torch.channels_last) \
        .requires_grad_(True)
    wt = k["w"].float().to(DEV).requires_grad_(True)   # fp32 leaf: dw stays fp32
    y = dwconv5x5(x, wt, stride)
    assert y.dtype == torch.bfloat16 and y.shape == (n, c, k["ho"], k["wo"])
    y.backward(k["dy"].to(DEV))
    assert tuple(wt.grad.shape) == (c, 1, 5, 5)
    assert tuple(x.grad.shape) == shape and x.grad.dtype == torch.bfloat16
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(-1, c), y2d)
    assert torch.equal(x.grad.permute(0, 2, 3, 1).reshape(-1, c), dx2d)
    assert torch.equal(wt.grad, dw25.t().reshape(c, 1, 5, 5))


def test_host_rejects_out_of_contract():
    from amdtrain import _C
    x12 = torch.zeros(2 * 4 * 4, 12, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(2 * 4 * 4, 16, device=DEV, dtype=torch.bfloat16)
    w25 = torch.zeros(25, 16, device=DEV, dtype=torch.bfloat16)
    for bad in [
        lambda: _C.dwconv5x5_fwd(x12, 2, 4, 4, 1, w25[:, :12].contiguous()),
        lambda: _C.dwconv5x5_fwd(x, 2, 4, 4, 3, w25),         # stride 3
        lambda: _C.dwconv5x5_fwd(x, 2, 4, 5, 1, w25),         # rows != N*H*W
        lambda: _C.dwconv5x5_fwd(x.float(), 2, 4, 4, 1, w25),  # dtype
        lambda: _C.dwconv5x5_dgrad(x, 2, 4, 4, 2, w25),       # dy rows for s2
        lambda: _C.dwconv5x5_wgrad(x, x[:16], 2, 4, 4, 1),    # x rows
    ]:
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


def _count(monkeypatch):
    import amdtrain.ops.conv as conv
    calls = {3: 0, 5: 0}
    for k, name in ((3, "dwconv3x3"), (5, "dwconv5x5")):
        def counted(x, weight, stride=1, k=k, real=getattr(conv, name)):
            calls[k] += 1
            return real(x, weight, stride)
        monkeypatch.setattr(conv, name, counted)
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    return calls


@pytest.mark.parametrize("stride", [1, 2])
def test_empty_batch(monkeypatch, stride):
    """N == 0 is served on the host: empty y and dx, zero dw."""
    from amdtrain.ops.conv import AmdConv2d
    calls = _count(monkeypatch)
    conv = AmdConv2d(16, 16, 5, stride=stride, padding=2, groups=16,
                     bias=False).to(DEV).to(torch.bfloat16)
    x = torch.zeros(0, 16, 5, 7, device=DEV, dtype=torch.bfloat16) \
        .requires_grad_(True)
    y = conv(x)
    assert calls == {3: 0, 5: 1}
    assert tuple(y.shape) == (0, 16) + _out_hw(5, 7, stride)
    assert y.dtype == torch.bfloat16
    y.backward(torch.zeros_like(y))
    torch.cuda.synchronize()
    assert tuple(x.grad.shape) == (0, 16, 5, 7)
    assert tuple(conv.weight.grad.shape) == (16, 1, 5, 5)
    assert (conv.weight.grad == 0).all()


@pytest.mark.parametrize("env,expect", [
    ({}, {3: 7, 5: 10}),
    ({"AMDTRAIN_DWCONV5X5": "0"}, {3: 7, 5: 0}),
    ({"AMDTRAIN_DWCONV": "miopen"}, {3: 0, 5: 0}),
])
def test_dispatch_mnasnet(monkeypatch, env, expect):
    from amdtrain.models import build_model
    calls = _count(monkeypatch)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    torch.manual_seed(0)
    m = build_model("mnasnet1_0", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert calls == expect


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_model_step(monkeypatch):
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD

    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(0)
    m = build_model("mnasnet1_0").to(DEV) \
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
    m.classifier[0].p = 0.0
    ref = build_model("mnasnet1_0")
    ref.load_state_dict({k: v.detach().cpu() for k, v in
                         m.state_dict().items()})
    ref.train()
    ref.classifier[0].p = 0.0
    out_ref = ref(x_cpu)
    torch.nn.functional.cross_entropy(out_ref, t_cpu).backward()
    g_ref = ref.classifier[1].weight.grad

    def gpu_pass():
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
            loss = crit(out, t)
        loss.backward()
        torch.cuda.synchronize()
        return (_rel(out.detach().float().cpu(), out_ref.detach()),
                _rel(m.classifier[1].weight.grad.float().cpu(), g_ref))

    e_custom = gpu_pass()
    monkeypatch.setenv("AMDTRAIN_DWCONV5X5", "0")
    e_lib = gpu_pass()
    print(f"(logits, classifier.1.weight.grad): e_custom {e_custom} "
          f"e_lib {e_lib}")
    assert e_custom[0] <= 2 * e_lib[0] and e_custom[1] <= 2 * e_lib[1]
