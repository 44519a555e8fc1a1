"""Per-group grouped 3x3 weight-gradient kernel (gconv_wgrad.hip).

Reference: the autograd dW of F.conv2d(groups=g) in float64 on the CPU over
bf16-valued x, w and gy, and its magnitude twin A (the same sum over absolute
values).  dW is fp32 and bf16 products are exact in fp32, so any fp32
summation order over M rows errs by at most (M-1) 2^-24 A to first order; all
shapes here have M <= 342, so per element

    |got - ref| <= 2^-14 A        (about 3x headroom).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CG = [(32, 8), (96, 12), (96, 6), (128, 4)]                  # S = 4, 8, 16, 32
GEOM = [(2, 9, 19, 1), (2, 9, 11, 2), (1, 10, 35, 2)]        # (N, H, W, stride)


@functools.lru_cache(maxsize=None)
def _case(c, groups, n, h, w, stride):
    """Seeded bf16-valued inputs, the float64 dW and its magnitude twin;
    computed once per shape, shared read-only."""
    g = torch.Generator().manual_seed(7919 * c + 131 * groups + 17 * w + stride)
    s = c // groups
    x = torch.randn(n, c, h, w, generator=g).bfloat16().double()
    wt = (torch.randn(c, s, 3, 3, generator=g) * (9 * s) ** -0.5) \
        .bfloat16().double()
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    gy = torch.randn(n, c, ho, wo, generator=g).bfloat16().double()
    dws = []
    for f in (lambda v: v, torch.abs):
        wv = wt.clone().requires_grad_(True)
        F.conv2d(f(x), wv, None, stride, 1, 1, groups).backward(f(gy))
        dws.append(wv.grad)
    return dict(x=x, w=wt, gy=gy, ref=dws[0], mag=dws[1])


def _rows(t):
    return t.float().cuda().bfloat16().permute(0, 2, 3, 1) \
        .reshape(-1, t.shape[1]).contiguous()


def _check(name, got, k):
    err = (got.double().cpu() - k["ref"]).abs()
    bound = 2.0 ** -14 * k["mag"]
    print(f"{name}: max err {err.max().item():.3e}, max err/bound "
          f"{(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert got.shape == k["ref"].shape and got.dtype == torch.float32
    assert (err <= bound).all(), f"{name}: {(err > bound).sum().item()} over"


@pytest.mark.parametrize("geom", GEOM)
@pytest.mark.parametrize("cg", CG)
def test_wgrad_vs_fp64(cg, geom):
    from amdtrain import _C
    k = _case(*cg, *geom)
    dw = _C.gconv3x3_wgrad(_rows(k["gy"]), _rows(k["x"]), *geom, cg[1], 0)
    assert dw.is_contiguous(memory_format=torch.channels_last)
    _check("dw", dw, k)


@pytest.mark.parametrize("nsplit", [1, 3, 8])
@pytest.mark.parametrize("cg", [(96, 12), (128, 4)])
def test_split_and_determinism(cg, nsplit):
    from amdtrain import _C
    k = _case(*cg, *GEOM[0])
    gy2d, x2d = _rows(k["gy"]), _rows(k["x"])
    a = _C.gconv3x3_wgrad(gy2d, x2d, *GEOM[0], cg[1], nsplit)
    b = _C.gconv3x3_wgrad(gy2d, x2d, *GEOM[0], cg[1], nsplit)
    _check(f"dw nsplit={nsplit}", a, k)
    assert torch.equal(a, b)


def test_routing(monkeypatch):
    from amdtrain import _C
    from amdtrain.ops.conv import _grouped_dw, conv3x3_grouped
    c, groups = 128, 4
    n, h, w, stride = GEOM[0]
    k = _case(c, groups, *GEOM[0])
    gy2d, x2d = _rows(k["gy"]), _rows(k["x"])

    def grad():
        cl = torch.channels_last
        x = k["x"].float().cuda().contiguous(memory_format=cl)
        wt = k["w"].float().cuda().contiguous(memory_format=cl) \
            .requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = conv3x3_grouped(x, wt, stride, groups)
        y.backward(k["gy"].float().cuda().bfloat16())
        return wt.grad

    new = grad()
    assert torch.equal(new, _C.gconv3x3_wgrad(gy2d, x2d, n, h, w, stride,
                                              groups))
    monkeypatch.setenv("AMDTRAIN_GCONV_WGRAD", "0")
    old = grad()
    assert torch.equal(old, _grouped_dw(_C, gy2d, x2d, n, h, w, stride, c,
                                        groups, True))
    _check("new route", new, k)
    _check("banded route", old, k)
    _check("new vs banded", new, dict(ref=old.double().cpu(), mag=k["mag"]))
    with pytest.raises(RuntimeError):      # S = 2
        _C.gconv3x3_wgrad(gy2d, x2d, n, h, w, stride, 64)
    with pytest.raises(RuntimeError):      # dY rows of another geometry
        _C.gconv3x3_wgrad(gy2d[:-1], x2d, n, h, w, stride, groups)
