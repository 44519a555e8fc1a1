"""Depthwise 3x3 stencil kernels (dwconv.hip) against fp64 references, their
dispatch through AmdConv2d, and a mobilenet_v2 training step.

Bounds (derived, not tuned).  ``A`` is the reference quantity with every
operand replaced by its absolute value, i.e. the sum of the absolute terms.

  y, dx:  |out - ref| <= 2^-8 |ref| + 2^-20 A
          one bf16 rounding is at most 2^-9 relative; at most 9 fp32
          additions of exact bf16 products cost at most 9 * 2^-24 * A.
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
    (2, 32, 14, 14),    # power-of-two C
    (2, 144, 15, 15),   # 18 packs, odd size, stride 2 on odd size
    (3, 40, 5, 3),      # W narrower than a strip, H != W, 3 images
    (1, 8, 1, 1),       # all taps but the centre are padding
    (2, 960, 7, 7),     # widest layer, last-stage size
    (1, 2056, 3, 2),    # 257 packs: second pack group of the wgrad blocks
]
CASES = [(s, st) for s in SHAPES for st in (1, 2)]


def _out_hw(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


@functools.lru_cache(maxsize=None)
def _case(shape, stride):
    """Seeded bf16-rounded operands and the fp64 CPU references; computed
    once per case and shared (read-only) by the tests."""
    n, c, h, w = shape
    ho, wo = _out_hw(h, w, stride)
    g = torch.Generator().manual_seed(1000 * c + 10 * h + stride)
    x = torch.randn(n, c, h, w, generator=g).bfloat16()
    dy = torch.randn(n, c, ho, wo, generator=g).bfloat16()
    wt = (torch.randn(c, 1, 3, 3, generator=g) / 3).bfloat16()

    def ref(xx, ww, gg):
        xx = xx.double().requires_grad_(True)
        ww = ww.double().requires_grad_(True)
        y = F.conv2d(xx, ww, None, stride, 1, 1, c)
        dx, dw = torch.autograd.grad(y, (xx, ww), gg.double())
        return y.detach(), dx, dw

    y, dx, dw = ref(x, wt, dy)
    ya, dxa, dwa = ref(x.abs(), wt.abs(), dy.abs())
    return dict(x=x, dy=dy, w=wt, y=y, dx=dx, dw=dw, ya=ya, dxa=dxa,
                dwa=dwa, ho=ho, wo=wo)


def _rows_gpu(t):
    """NCHW CPU bf16 -> [N*H*W, C] contiguous rows on the GPU."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous().to(DEV)


def _nchw64(t2d, n, h, w, c):
    return t2d.view(n, h, w, c).permute(0, 3, 1, 2).double().cpu()


def _w9(wt):
    c = wt.shape[0]
    return wt.reshape(c, 9).t().contiguous().to(DEV)


def _run_kernels(shape, stride):
    from amdtrain import _C
    n, c, h, w = shape
    k = _case(shape, stride)
    x2d, dy2d, w9 = _rows_gpu(k["x"]), _rows_gpu(k["dy"]), _w9(k["w"])
    y2d = _C.dwconv3x3_fwd(x2d, n, h, w, stride, w9)
    dx2d = _C.dwconv3x3_dgrad(dy2d, n, h, w, stride, w9)
    dw9 = _C.dwconv3x3_wgrad(dy2d, x2d, n, h, w, stride)
    torch.cuda.synchronize()
    return y2d, dx2d, dw9


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
    y2d, dx2d, dw9 = _run_kernels(shape, stride)

    assert tuple(y2d.shape) == (n * ho * wo, c) and y2d.dtype == torch.bfloat16
    assert tuple(dx2d.shape) == (n * h * w, c) and dx2d.dtype == torch.bfloat16
    assert tuple(dw9.shape) == (9, c) and dw9.dtype == torch.float32

    y = _nchw64(y2d, n, ho, wo, c)
    dx = _nchw64(dx2d, n, h, w, c)
    dw = dw9.t().reshape(c, 1, 3, 3).double().cpu()
    L = n * ho * wo
    assert L <= 2000
    _check("y", y, k["y"], 2.0 ** -8 * k["y"].abs() + 2.0 ** -20 * k["ya"])
    _check("dx", dx, k["dx"],
           2.0 ** -8 * k["dx"].abs() + 2.0 ** -20 * k["dxa"])
    _check("dw", dw, k["dw"], L * 2.0 ** -23 * k["dwa"])


@pytest.mark.parametrize("stride", [1, 2])
def test_autograd_wrapper_matches_kernels(stride):
    """dwconv3x3() on the GPU is the three kernels: same bits, dw returned
    as [C, 1, 3, 3]."""
    from amdtrain.ops.conv import dwconv3x3
    shape = (2, 144, 15, 15)
    n, c, h, w = shape
    k = _case(shape, stride)
    y2d, dx2d, dw9 = _run_kernels(shape, stride)
    x = k["x"].to(DEV).contiguous(memory_format=torch.channels_last) \
        .requires_grad_(True)
    wt = k["w"].float().to(DEV).requires_grad_(True)   # fp32 leaf: dw stays fp32
    y = dwconv3x3(x, wt, stride)
    assert y.dtype == torch.bfloat16
    assert tuple(y.shape) == (n, c, k["ho"], k["wo"])
    y.backward(k["dy"].to(DEV))
    assert tuple(wt.grad.shape) == (c, 1, 3, 3)
    assert tuple(x.grad.shape) == shape and x.grad.dtype == torch.bfloat16
    assert torch.equal(y.permute(0, 2, 3, 1).reshape(-1, c), y2d)
    assert torch.equal(x.grad.permute(0, 2, 3, 1).reshape(-1, c), dx2d)
    assert torch.equal(wt.grad, dw9.t().reshape(c, 1, 3, 3))


@pytest.mark.parametrize("stride", [1, 2])
def test_bitwise_deterministic(stride):
    a = _run_kernels((2, 144, 15, 15), stride)
    b = _run_kernels((2, 144, 15, 15), stride)
    for name, p, q in zip(("y", "dx", "dw"), a, b):
        assert torch.equal(p, q), name


def test_host_rejects_out_of_contract():
    """A shape outside the contract fails on the host."""
    from amdtrain import _C
    x = torch.zeros(2 * 4 * 4, 12, device=DEV, dtype=torch.bfloat16)
    w9 = torch.zeros(9, 12, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_fwd(x, 2, 4, 4, 1, w9)              # C % 8 != 0
    x = torch.zeros(2 * 4 * 4, 16, device=DEV, dtype=torch.bfloat16)
    w9 = torch.zeros(9, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_fwd(x, 2, 4, 4, 3, w9)              # stride 3
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_fwd(x, 2, 4, 5, 1, w9)              # rows != N*H*W
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_fwd(x.float(), 2, 4, 4, 1, w9)      # dtype
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_dgrad(x, 2, 4, 4, 2, w9)            # dy rows for s2
    with pytest.raises(RuntimeError):
        _C.dwconv3x3_wgrad(x, x[:16], 2, 4, 4, 1)        # x rows
    torch.cuda.synchronize()


def _count_dwconv(monkeypatch):
    import amdtrain.ops.conv as conv
    calls = []
    real = conv.dwconv3x3

    def counted(x, weight, stride=1):
        calls.append(tuple(weight.shape))
        return real(x, weight, stride)

    monkeypatch.setattr(conv, "dwconv3x3", counted)
    return calls


def test_dispatch_mobilenet(monkeypatch):
    from amdtrain.models import build_model
    calls = _count_dwconv(monkeypatch)
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    monkeypatch.delenv("AMDTRAIN_DWCONV", raising=False)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert len(calls) == 17
    del calls[:]
    monkeypatch.setenv("AMDTRAIN_DWCONV", "miopen")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    assert len(calls) == 0


def test_host_guard_c12(monkeypatch):
    """C = 12 is not a whole number of 8-channel packs: AmdConv2d keeps it
    on the library path and the result is still a depthwise conv."""
    from amdtrain.ops.conv import AmdConv2d
    calls = _count_dwconv(monkeypatch)
    monkeypatch.delenv("AMDTRAIN_DWCONV", raising=False)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 12, 9, 9, generator=g).bfloat16()
    conv = AmdConv2d(12, 12, 3, padding=1, groups=12, bias=False)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(12, 1, 3, 3, generator=g) / 3)
                          .bfloat16())
    wt = conv.weight.detach().clone()
    conv = conv.to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        y = conv(x.to(DEV).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert len(calls) == 0
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1, 1, 12)
    refa = F.conv2d(x.double().abs(), wt.double().abs(), None, 1, 1, 1, 12)
    # the library may round every partial sum to bf16: 9 roundings of at
    # most 2^-9 of the absolute sum, plus the output rounding
    _check("y_c12", y.double().cpu(), ref,
           2.0 ** -8 * ref.abs() + 9 * 2.0 ** -9 * refa)


@pytest.mark.parametrize("stride", [1, 2])
def test_empty_batch(monkeypatch, stride):
    """N == 0 is served on the host: empty y and dx, zero dw, as the
    library path gives."""
    from amdtrain.ops.conv import AmdConv2d
    calls = _count_dwconv(monkeypatch)
    monkeypatch.delenv("AMDTRAIN_DWCONV", raising=False)
    conv = AmdConv2d(16, 16, 3, stride=stride, padding=1, groups=16,
                     bias=False).to(DEV).to(torch.bfloat16)
    x = torch.zeros(0, 16, 5, 7, device=DEV, dtype=torch.bfloat16) \
        .requires_grad_(True)
    y = conv(x)
    ho, wo = _out_hw(5, 7, stride)
    assert len(calls) == 1
    assert tuple(y.shape) == (0, 16, ho, wo) and y.dtype == torch.bfloat16
    y.backward(torch.zeros_like(y))
    torch.cuda.synchronize()
    assert tuple(x.grad.shape) == (0, 16, 5, 7)
    assert tuple(conv.weight.grad.shape) == (16, 1, 3, 3)
    assert (conv.weight.grad == 0).all()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_model_step(monkeypatch):
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD

    monkeypatch.delenv("AMDTRAIN_DWCONV", raising=False)
    torch.manual_seed(0)
    m = build_model("mobilenet_v2").to(DEV) \
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

    # fp32 CPU copy of the weights as they stand.  Dropout draws a different
    # mask on every device and call, so it is switched off for the
    # comparison; everything else stays in train mode.
    m.classifier[0].p = 0.0
    ref = build_model("mobilenet_v2")
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
    monkeypatch.setenv("AMDTRAIN_DWCONV", "miopen")
    e_lib = gpu_pass()
    print(f"logits: e_custom {e_custom[0]:.4e} e_lib {e_lib[0]:.4e}")
    print(f"classifier.1.weight.grad: e_custom {e_custom[1]:.4e} "
          f"e_lib {e_lib[1]:.4e}")
    assert e_custom[0] <= 2 * e_lib[0]
    assert e_custom[1] <= 2 * e_lib[1]
