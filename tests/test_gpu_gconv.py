"""Per-group grouped 3x3 kernel (gconv.hip): forward, input and weight
gradient, statistics partials, determinism and the AmdConv2d dispatch.

Reference: F.conv2d(groups=g) in float64 on the CPU over the bf16-rounded x
and weight; its autograd gives dx and dW.  With A the same sum over
magnitudes, per element

    |got - ref| <= 2^-8 |ref| + 2^-14 A

(bf16 rounding of the result with 2x headroom; fp32 accumulation of
K <= 288 products, K 2^-24 A worst case, with ~4x headroom; the fp32 split
sum of the weight gradient over <= 342 rows stays inside the same form).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CG = [(32, 8), (96, 12), (96, 6), (128, 4)]      # S = 4, 8, 16, 32
GEOM = [(2, 9, 19, 1), (2, 9, 11, 2)]            # (N, H, W, stride)


@functools.lru_cache(maxsize=None)
def _case(c, groups, n, h, w, stride):
    """Seeded bf16-valued inputs with their float64 references and
    magnitude sums; computed once per shape, shared read-only."""
    g = torch.Generator().manual_seed(7919 * c + 131 * groups + 17 * w + stride)
    s = c // groups
    x = torch.randn(n, c, h, w, generator=g).bfloat16().double()
    wt = (torch.randn(c, s, 3, 3, generator=g) * (9 * s) ** -0.5) \
        .bfloat16().double()
    out = {}
    for key, f in (("ref", lambda v: v), ("mag", torch.abs)):
        xv = f(x).detach().clone().requires_grad_(True)
        wv = f(wt).detach().clone().requires_grad_(True)
        y = F.conv2d(xv, wv, None, stride, 1, 1, groups)
        if key == "ref":
            gy = torch.randn(y.shape, generator=g).bfloat16().double()
        y.backward(f(gy))
        out[key] = (y.detach(), xv.grad, wv.grad)
    return dict(x=x, w=wt, gy=gy, **out)


def _check(name, got, ref, mag):
    err = (got.detach().double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -14 * mag
    print(f"{name}: max err {err.max().item():.3e}, max err/bound "
          f"{(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert got.shape == ref.shape and (err <= bound).all(), \
        f"{name}: {(err > bound).sum().item()} over the bound"


def _dev(t):
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def _rows(t):
    return _dev(t).bfloat16().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("geom", GEOM)
@pytest.mark.parametrize("cg", CG)
def test_fwd_dgrad_wgrad_vs_fp64(cg, geom):
    from amdtrain.ops.conv import conv3x3_grouped
    k = _case(*cg, *geom)
    x, w = _dev(k["x"]).requires_grad_(True), _dev(k["w"]).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv3x3_grouped(x, w, geom[3], cg[1])
    y.backward(_dev(k["gy"]).bfloat16())
    for name, got, i in (("y", y, 0), ("dx", x.grad, 1), ("dw", w.grad, 2)):
        _check(name, got, k["ref"][i], k["mag"][i])


@pytest.mark.parametrize("cg", [(32, 8), (96, 6)])
def test_stats_partials(cg):
    from amdtrain import _C
    n, h, w, stride = GEOM[0]
    k = _case(*cg, n, h, w, stride)
    c = cg[0]
    packed = _C.gconv3x3_pack(_dev(k["w"]).bfloat16(), cg[1], False)
    _, parts = _C.gconv3x3_fwd(_rows(k["x"]), n, h, w, stride, packed, cg[1],
                               True)
    assert parts.dtype == torch.float32 and parts.shape[1] == 2 * c
    assert parts.shape[0] >= 2
    got = parts.double().sum(0).cpu()
    ref, mag = k["ref"][0], k["mag"][0]
    for name, g_, r_, b_ in (
            ("sum", got[:c], ref.sum((0, 2, 3)),
             2.0 ** -12 * mag.sum((0, 2, 3))),
            ("sumsq", got[c:], (ref ** 2).sum((0, 2, 3)),
             2.0 ** -11 * (mag ** 2).sum((0, 2, 3)))):
        err = (g_ - r_).abs()
        print(f"{name}: max err/bound {(err / b_).max().item():.3f}")
        assert (err <= b_).all(), name


@pytest.mark.parametrize("geom", GEOM)
def test_deterministic(geom):
    from amdtrain import _C
    c, groups = 96, 12
    n, h, w, stride = geom
    k = _case(c, groups, *geom)
    wt = _dev(k["w"]).bfloat16()
    x2d, gy2d = _rows(k["x"]), _rows(k["gy"])
    runs = []
    for _ in range(2):
        y, parts = _C.gconv3x3_fwd(x2d, n, h, w, stride,
                                   _C.gconv3x3_pack(wt, groups, False),
                                   groups, True)
        dx = _C.gconv3x3_dgrad(gy2d, n, h, w, stride,
                               _C.gconv3x3_pack(wt, groups, True), groups)
        runs.append((y, parts, dx))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_dispatch(monkeypatch):
    from amdtrain import _C
    from amdtrain.ops.conv import (AmdConv2d, conv3x3_grouped,
                                   conv3x3_grouped_mfma, conv3x3_mfma)
    torch.manual_seed(0)

    def run(conv, x):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return conv(x)

    def layer(c, groups):
        conv = AmdConv2d(c, c, 3, padding=1, groups=groups, bias=False) \
            .cuda().to(memory_format=torch.channels_last)
        x = torch.randn(2, c, 9, 19, device="cuda") \
            .contiguous(memory_format=torch.channels_last)
        return conv, x

    conv, x = layer(64, 16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        new = conv3x3_grouped(x, conv.weight, 1, 16)
        old = conv3x3_grouped_mfma(x, conv.weight, 1, 16)
    assert torch.equal(run(conv, x), new)
    monkeypatch.setenv("AMDTRAIN_GCONV", "0")
    assert torch.equal(run(conv, x), old)
    # outside the contract: groups == 1 and S = 64 ignore the switch
    for c, groups in ((64, 1), (128, 2)):
        conv, x = layer(c, groups)
        monkeypatch.setenv("AMDTRAIN_GCONV", "0")
        off = run(conv, x)
        monkeypatch.setenv("AMDTRAIN_GCONV", "1")
        assert torch.equal(run(conv, x), off)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            want = conv3x3_mfma(x, conv.weight, 1) if groups == 1 else \
                conv3x3_grouped_mfma(x, conv.weight, 1, groups)
        assert torch.equal(off, want)
    # S = 2 is refused on the host
    x2d = torch.zeros(2 * 9 * 19, 32, device="cuda", dtype=torch.bfloat16)
    packed = _C.gconv3x3_pack(torch.zeros(32, 4, 3, 3, device="cuda",
                                          dtype=torch.bfloat16), 8, False)
    with pytest.raises(RuntimeError):
        _C.gconv3x3_fwd(x2d, 2, 9, 19, 1, packed, 16, True)
