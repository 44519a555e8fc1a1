"""Direct 3x3 stride-2 RGB stem kernels (stem3x3.hip) against fp64, their
determinism, the AmdConv2d routing, the host contract and an mnasnet0_75 step.

Reference: fp64 F.conv2d on the bf16 input values, on the CPU.  With
S = conv(|x|, |w|), K = 27 and M = N*Ho*Wo the bounds are derived as in
test_gpu_pwconv.py, not measured:

  y:      |y - ref| <= 2^-8 |ref| + 28 2^-23 S
  stats, partial rows summed in fp64:
          |sum - sum ref|     <= (27 + M)     2^-23 sum S
          |sumsq - sum ref^2| <= (54 + M + 2) 2^-23 sum S^2
  dW:     |dW - ref| <= (M + 1) 2^-23 (|dY|^T |Xcol|)

x is a slice of a larger buffer whose images before and after are NaN, so a
halo read that is clamped instead of zero-filled shows in y or dW.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U23 = 2.0 ** -23
ENVS = ("AMDTRAIN_STEM3X3", "AMDTRAIN_CONVSTEM", "AMDTRAIN_FUSE_BNSTATS")

# stem3x3.hip tiles 8 x 32 output pixels (S3_TH x S3_TW).  19 x 69 gives
# Ho x Wo = 10 x 35: more than one tile each way, the last one ragged (2 rows,
# 3 columns); odd sizes put the last input row and column outside the image
# and send x down the element staging route.  (1, 17, 40) and (1, 5, 136)
# take the 16-byte route, the latter over three tiles in a row.
HBIG, WBIG = 19, 69
SHAPES = [(1, 1, 1), (2, 9, 11), (1, 17, 40), (2, HBIG, WBIG), (1, 5, 136)]
COUTS = [8, 24, 32, 40, 64]


def _check(name, out, ref, bound):
    out = out.detach().double().cpu()
    err = (out - ref).abs()
    print(f"{name}: max err {err.max().item():.3e}, max err/bound "
          f"{(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert out.shape == ref.shape, name
    assert torch.isfinite(out).all(), name
    assert (err <= bound).all(), \
        f"{name}: {(err > bound).sum().item()} elements over the bound"


@functools.lru_cache(maxsize=None)
def _case(n, h, w, cout):
    """Seeded bf16 operands and the fp64 reference, once per shape."""
    g = torch.Generator().manual_seed(10007 * h + 101 * w + cout)
    x = torch.randn(n, 3, h, w, generator=g).bfloat16()
    wt = (torch.randn(cout, 3, 3, 3, generator=g) * 27 ** -0.5).bfloat16()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    go = torch.randn(n, cout, ho, wo, generator=g).bfloat16()
    wd = wt.double().requires_grad_(True)
    y = F.conv2d(x.double(), wd, None, 2, 1)
    y.backward(go.double())
    wa = wt.double().abs().requires_grad_(True)
    s = F.conv2d(x.double().abs(), wa, None, 2, 1)
    s.backward(go.double().abs())
    return dict(x=x, w=wt, go=go, m=n * ho * wo, y=y.detach(), s=s.detach(),
                dw=wd.grad, s_dw=wa.grad)


def _rows(t):
    """[N, C, H, W] -> contiguous channels-last rows on the GPU."""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _x_between_nans(k):
    n, _, h, w = k["x"].shape
    big = torch.full((n + 2, h, w, 3), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    big[1:n + 1] = _rows(k["x"])
    return big[1:n + 1]


# 1. kernels against fp64
@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_kernels_vs_fp64(n, h, w, cout, want_stats):
    from amdtrain import _C
    k = _case(n, h, w, cout)
    m, x = k["m"], _x_between_nans(k)
    y2d, stats = _C.stem3x3_fwd(x, k["w"].to(DEV), want_stats)
    dw = _C.stem3x3_wgrad(_rows(k["go"]).view(m, cout), x)
    torch.cuda.synchronize()
    assert y2d.dtype == torch.bfloat16 and tuple(y2d.shape) == (m, cout)
    y = y2d.view(n, *k["y"].shape[2:], cout).permute(0, 3, 1, 2)
    _check("y", y, k["y"], 2.0 ** -8 * k["y"].abs() + 28 * U23 * k["s"])
    assert dw.dtype == torch.float32 and tuple(dw.shape) == (cout, 27)
    _check("dw", dw.view(cout, 3, 3, 3).permute(0, 3, 1, 2), k["dw"],
           (m + 1) * U23 * k["s_dw"])
    if not want_stats:
        assert stats.numel() == 0
        return
    assert stats.dtype == torch.float32 and stats.size(1) == 2 * cout
    tot = stats.double().cpu().sum(0)
    _check("sum", tot[:cout], k["y"].sum((0, 2, 3)),
           (27 + m) * U23 * k["s"].sum((0, 2, 3)))
    _check("sumsq", tot[cout:], (k["y"] ** 2).sum((0, 2, 3)),
           (54 + m + 2) * U23 * (k["s"] ** 2).sum((0, 2, 3)))


# 2. determinism: fixed reduction order, no atomics
def test_wgrad_bitwise_deterministic():
    from amdtrain import _C
    k = _case(2, HBIG, WBIG, 40)
    x, go = _x_between_nans(k), _rows(k["go"]).view(k["m"], 40)
    assert torch.equal(_C.stem3x3_wgrad(go, x), _C.stem3x3_wgrad(go, x))


# 3. routing and host contract
@pytest.mark.parametrize("cout,mode,expect", [
    (24, None, 1), (24, "0", 0), (24, "all", 1),
    (32, None, 0), (32, "0", 0), (32, "all", 1)])
def test_routing(monkeypatch, cout, mode, expect):
    import amdtrain.ops.conv as conv_mod
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    if mode is not None:
        monkeypatch.setenv("AMDTRAIN_STEM3X3", mode)
    calls = []
    real = conv_mod.conv_stem3x3
    monkeypatch.setattr(conv_mod, "conv_stem3x3",
                        lambda *a: calls.append(1) or real(*a))
    k = _case(2, 9, 11, cout)
    conv = conv_mod.AmdConv2d(3, cout, 3, 2, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(k["w"].float())
    conv = conv.to(DEV)
    x = k["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv(x)
    y.backward(k["go"].to(DEV))
    torch.cuda.synchronize()
    assert len(calls) == expect
    assert (getattr(y, "_amdtrain_bn_stats", None) is not None) == bool(expect)
    assert torch.isfinite(y).all() and torch.isfinite(conv.weight.grad).all()
    if expect:
        _check("y", y, k["y"], 2.0 ** -8 * k["y"].abs() + 28 * U23 * k["s"])
        _check("dw", conv.weight.grad, k["dw"],
               (k["m"] + 1) * U23 * k["s_dw"])


def test_host_contract():
    from amdtrain import _C

    def z(*shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=DEV)

    for cout, cin in [(12, 3), (72, 3), (8, 4)]:
        with pytest.raises(RuntimeError):
            _C.stem3x3_fwd(z(1, 4, 4, cin), z(cout, cin, 3, 3), False)
        with pytest.raises(RuntimeError):
            _C.stem3x3_wgrad(z(4, cout), z(1, 4, 4, cin))
    with pytest.raises(RuntimeError):
        _C.stem3x3_fwd(z(1, 4, 4, 3).float(), z(8, 3, 3, 3), False)
    y, stats = _C.stem3x3_fwd(z(0, 4, 4, 3), z(8, 3, 3, 3), True)  # no launch
    assert tuple(y.shape) == (0, 8) and stats.numel() == 0
    assert (_C.stem3x3_wgrad(z(0, 8), z(0, 4, 4, 3)) == 0).all()
    torch.cuda.synchronize()


# 4. model step
def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_model_step(monkeypatch):
    from amdtrain.models import mnasnet0_75
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(0)
    m = mnasnet0_75().to(DEV) \
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
    ref = mnasnet0_75()
    ref.load_state_dict({k: v.detach().cpu() for k, v in
                         m.state_dict().items()})
    ref.train()
    ref.classifier[0].p = 0.0
    out_ref = ref(x_cpu)
    F.cross_entropy(out_ref, t_cpu).backward()
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
    monkeypatch.setenv("AMDTRAIN_STEM3X3", "0")
    e_lib = gpu_pass()
    print(f"(logits, classifier.1.weight.grad): e_custom {e_custom} "
          f"e_lib {e_lib}")
    assert e_custom[0] <= 2 * e_lib[0] and e_custom[1] <= 2 * e_lib[1]
