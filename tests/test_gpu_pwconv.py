"""Thin pointwise (1x1 conv) GEMM kernel (pwconv.hip): pw_gemm against fp64,
the _ConvPw layer, the conv -> BN statistics partials, the mobilenet_v2
dispatch, determinism, the host contract and 64-bit offsets.

Reference: fp64 arithmetic on the bf16 input values (products are exact).
With ref = A B^T and S = |A| |B|^T the bounds are derived, not measured:

  C:           |C - ref| <= 2^-8 |ref| + (K+1) 2^-23 S
               (bf16 rounding of the output; fp32 accumulation of K terms)
  statistics,  summed over the partial rows in fp64:
               |sum   - sum_m ref|   <= (K+M)    2^-23 sum_m S
               |sumsq - sum_m ref^2| <= (2K+M+2) 2^-23 sum_m S^2
  layer dW (fp32): |dW - ref| <= (M+1) 2^-23 (|dY|^T |X|)
  layer dX:    the C bound with (K, N) swapped

Inputs are random and asymmetric (N != K, B not symmetric), so a transposed
C map cannot pass.  Every test that calls pw_gemm fails without the kernel.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U23 = 2.0 ** -23

LAYER_PAIRS = [(32, 16), (16, 32), (16, 96), (96, 16), (96, 24), (24, 96),
               (24, 144), (144, 24), (144, 32), (32, 144)]
# ragged last k-pack; K and N off the 16 grid; min-K with max-N
EXTRA_PAIRS = [(8, 8), (40, 56), (8, 160)]


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


@functools.lru_cache(maxsize=None)
def _case(m, k, n):
    """Seeded bf16 operands and their fp64 reference; computed once per
    shape and shared (read-only) by the tests."""
    g = torch.Generator().manual_seed(1000003 * m + 1009 * k + n)
    a = torch.randn(m, k, generator=g).bfloat16()
    b = (torch.randn(n, k, generator=g) * k ** -0.5).bfloat16()
    ad, bd = a.double(), b.double()
    ref = ad @ bd.t()
    s = ad.abs() @ bd.abs().t()
    return dict(m=m, k=k, n=n, a=a, b=b, ref=ref, s=s)


def _c_bound(ref, s, k):
    return 2.0 ** -8 * ref.abs() + (k + 1) * U23 * s


def _check_c(c, case):
    assert c.dtype == torch.bfloat16
    _check("C", c, case["ref"], _c_bound(case["ref"], case["s"], case["k"]))


def _check_stats(stats, case):
    m, k, n = case["m"], case["k"], case["n"]
    ref, s = case["ref"], case["s"]
    assert stats.dtype == torch.float32 and stats.size(1) == 2 * n
    tot = stats.double().cpu().sum(0)
    assert torch.isfinite(stats).all()
    _check("sum", tot[:n], ref.sum(0), (k + m) * U23 * s.sum(0))
    _check("sumsq", tot[n:], (ref * ref).sum(0),
           (2 * k + m + 2) * U23 * (s * s).sum(0))


def _run_kernel(case, want_stats, max_blocks=-1, nan_tail=True):
    """A is the first M rows of a larger buffer whose other rows are NaN: a
    tail row that is clamped instead of masked shows in C or the sums."""
    from amdtrain import _C
    m, k = case["m"], case["k"]
    big = torch.full((m + 300, k), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    big[:m] = case["a"].to(DEV)
    a = big[:m] if nan_tail else big[:m].clone()
    c, stats = _C.pw_gemm(a, case["b"].to(DEV), want_stats, max_blocks)
    torch.cuda.synchronize()
    return c, stats


# 1. kernel against fp64
@pytest.mark.parametrize("want_stats", [False, True])
@pytest.mark.parametrize("k,n", LAYER_PAIRS + EXTRA_PAIRS)
def test_kernel_vs_fp64(k, n, want_stats):
    case = _case(777, k, n)
    c, stats = _run_kernel(case, want_stats)
    assert tuple(c.shape) == (777, n)
    _check_c(c, case)
    if want_stats:
        _check_stats(stats, case)
    else:
        assert stats.numel() == 0


# 2. edge M, and a capped grid whose blocks stride over several tiles
@pytest.mark.parametrize("m", [1, 15, 129])
@pytest.mark.parametrize("k,n", [(32, 16), (24, 144), (144, 24)])
def test_edge_m(m, k, n):
    case = _case(m, k, n)
    c, stats = _run_kernel(case, True)
    _check_c(c, case)
    _check_stats(stats, case)


def test_capped_grid_strides_over_tiles():
    case = _case(1000, 24, 144)
    c, stats = _run_kernel(case, True, max_blocks=2)
    assert stats.size(0) == 2
    _check_c(c, case)
    _check_stats(stats, case)


# 3. layer
def _spy(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)

    monkeypatch.setattr(owner, name, counted)
    return calls


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _layer_case(cin, cout):
    g = torch.Generator().manual_seed(7919 * cin + cout)
    x = torch.randn(2, cin, 5, 7, generator=g).bfloat16()
    w = (torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5).bfloat16()
    go = torch.randn(2, cout, 5, 7, generator=g).bfloat16()
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    y = F.conv2d(xd, wd)
    y.backward(go.double())
    xa, wa, ga = x.double().abs(), w.double().abs(), go.double().abs()
    m = 2 * 5 * 7
    # |dY|^T |X| and |dY| |W| as the gradients of the all-absolute conv
    xa.requires_grad_(True)
    wa.requires_grad_(True)
    F.conv2d(xa, wa).backward(ga)
    return dict(x=x, w=w, go=go, m=m, y=y.detach(),
                s_y=F.conv2d(xa.detach(), wa.detach()), dx=xd.grad,
                s_dx=xa.grad, dw=wd.grad, s_dw=wa.grad)


def _make_layer(k, cin, cout):
    """fp32 master weight holding bf16 values, run under autocast: the weight
    gradient then arrives in fp32, as in training."""
    from amdtrain.ops.conv import AmdConv2d
    conv = AmdConv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(k["w"].float())
    return conv.to(DEV)


def _run_layer(k, cin, cout, x_grad=True):
    conv = _make_layer(k, cin, cout)
    x = _nhwc(k["x"]).requires_grad_(x_grad)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv(x)
    y.backward(_nhwc(k["go"]))
    torch.cuda.synchronize()
    return y, x.grad, conv.weight.grad


@pytest.mark.parametrize("cin,cout", [(32, 16), (16, 96), (144, 24),
                                      (24, 144)])
def test_layer(monkeypatch, cin, cout):
    from amdtrain import _C
    import amdtrain.ops.conv as conv_mod
    monkeypatch.delenv("AMDTRAIN_PWCONV", raising=False)
    monkeypatch.delenv("AMDTRAIN_CONV1X1", raising=False)
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", "1")
    thin = _spy(monkeypatch, conv_mod, "conv1x1_thin")
    pw = _spy(monkeypatch, _C, "pw_gemm")
    k = _layer_case(cin, cout)
    y, dx, dw = _run_layer(k, cin, cout)
    assert len(thin) == 1 and len(pw) == 2
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    assert dw.dtype == torch.float32
    assert getattr(y, "_amdtrain_bn_stats", None) is not None
    assert y._amdtrain_bn_stats.size(1) == 2 * cout
    _check("y", y, k["y"], _c_bound(k["y"], k["s_y"], cin))
    _check("dx", dx, k["dx"], _c_bound(k["dx"], k["s_dx"], cout))
    _check("dw", dw, k["dw"], (k["m"] + 1) * U23 * k["s_dw"])
    # input without a gradient: the dgrad launch is not made
    del pw[:]
    y2, dx2, dw2 = _run_layer(k, cin, cout, x_grad=False)
    assert len(pw) == 1 and dx2 is None
    assert torch.equal(y2, y) and torch.equal(dw2, dw)
    # no partials with the fusion off
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", "0")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y3 = _make_layer(k, cin, cout)(_nhwc(k["x"]))
    assert getattr(y3, "_amdtrain_bn_stats", None) is None
    assert torch.equal(y3, y)


# 4. conv -> BN from the partials (the check of
# test_gpu_bn_anyc.py::test_stats_from_conv_partials at the thin widths)
@functools.lru_cache(maxsize=None)
def _partials_inputs(cin, cout):
    """Inputs of that check, drawn as it draws them.  Its bound grants the
    partials one u S (u = 2^-9, S = |scale||x| + |shift|) for taking the
    statistics from the conv's unrounded output instead of its bf16
    rounding.  That holds unless a channel's shift = bias - mean * scale
    cancels to nearly nothing, where S no longer sees the term
    |scale| * delta(mean) that the move of the mean costs (measured on the
    32 -> 192 gemm_bt path as well: 1 of 12 seeds, 1.9x the bound; the
    thin 16 -> 96 path: 1 of 12, 1.02x, and 1.09x at seed 16096).  The premise is therefore checked on the reference side alone,
    in fp64, never on a kernel's result: with x the correctly rounded conv
    output, v from the statistics of the unrounded output and v from those
    of x differ by at most u S in every element.  The seed is the first
    from 1000 * cin + cout upward whose draw meets it."""
    for seed in range(1000 * cin + cout, 1000 * cin + cout + 64):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(cout, cin, 1, 1, generator=g)
             * cin ** -0.5).bfloat16()
        xin = torch.randn(2, cin, 6, 6, generator=g).bfloat16()
        go = torch.randn(2, cout, 6, 6, generator=g).bfloat16()
        weight = torch.rand(cout, generator=g) * 2 + 2
        bias = torch.rand(cout, generator=g) * 2 + 1
        exact = F.conv2d(xin.double(), w.double())
        x = exact.bfloat16().double()

        def affine(t):
            mean = t.mean((0, 2, 3))
            var = (t * t).mean((0, 2, 3)) - mean * mean
            scale = weight.double() * (var + 1e-5).rsqrt()
            shift = bias.double() - mean * scale
            pc = lambda u: u.view(1, -1, 1, 1)  # noqa: E731
            return (pc(scale) * x + pc(shift),
                    pc(scale.abs()) * x.abs() + pc(shift.abs()))

        (v_x, s_x), (v_e, _) = affine(x), affine(exact)
        if ((v_e - v_x).abs() <= 2.0 ** -9 * s_x).all():
            return dict(w=w, xin=xin, go=go, weight=weight, bias=bias)
    raise AssertionError("no draw meets the premise of the bound")


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("cin,cout,act", [(16, 96, "relu6"),
                                          (144, 24, "none")])
def test_stats_from_thin_conv_partials(monkeypatch, cin, cout, act, fuse):
    import test_gpu_bn_anyc as bnt
    from amdtrain import _C
    from amdtrain.ops import fused
    from amdtrain.ops.conv import AmdConv2d
    monkeypatch.delenv("AMDTRAIN_PWCONV", raising=False)
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", fuse)
    lib = bnt._spy_library(monkeypatch)
    from_parts = bnt._spy(monkeypatch, _C, "batch_norm_fwd_train_from_parts")
    pw = bnt._spy(monkeypatch, _C, "pw_gemm")
    d = _partials_inputs(cin, cout)
    xin, go, weight, bias = d["xin"], d["go"], d["weight"], d["bias"]
    conv = AmdConv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(d["w"])
    conv = conv.to(DEV).to(torch.bfloat16)
    rm0 = torch.zeros(cout)
    rv0 = torch.ones(cout)
    with torch.no_grad():
        xc = conv(bnt._nhwc(xin))
    assert len(pw) == 1
    assert (getattr(xc, "_amdtrain_bn_stats", None) is not None) \
        == (fuse == "1")
    ref = bnt._reference(xc.cpu(), None, go, weight, bias, rm0, rv0, act,
                         margin0=1e-2, margin6=1e-2)
    bnt._assert_shares(ref, act)
    k = dict(shape=(2, cout, 6, 6), dtype=torch.bfloat16, act=act,
             x=None, z=None, weight=weight, bias=bias, rm0=rm0, rv0=rv0,
             ref=ref)
    bn = bnt._make_bn(k).train()
    xc.requires_grad_(True)
    y = fused.batch_norm(xc, bn, relu6=act == "relu6")
    (y.float() * bnt._nhwc(ref["go"].float())).sum().backward()
    torch.cuda.synchronize()
    assert len(from_parts) == (1 if fuse == "1" else 0)
    assert lib == ([], [])
    bnt._check_all(k, dict(y=y.detach(), gx=xc.grad), stats=False)


# 5. dispatch: no conv of mobilenet_v2 uses a library
@pytest.mark.parametrize("flag,expect", [(None, (0, 1, 27, 7)),
                                         ("0", (3, 5, 27, 0))])
def test_dispatch_mobilenet(monkeypatch, flag, expect):
    import amdtrain.ops.conv as conv_mod
    from amdtrain.models import build_model
    for name in ("AMDTRAIN_CONV1X1", "AMDTRAIN_CONVSTEM", "AMDTRAIN_DWCONV",
                 "AMDTRAIN_PWCONV"):
        monkeypatch.delenv(name, raising=False)
    if flag is not None:
        monkeypatch.setenv("AMDTRAIN_PWCONV", flag)
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    lib = _spy(monkeypatch, torch.nn.functional, "conv2d")
    generic = _spy(monkeypatch, conv_mod, "conv_stem_mfma")
    gemm = _spy(monkeypatch, conv_mod, "conv1x1_mfma")
    thin = _spy(monkeypatch, conv_mod, "conv1x1_thin")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    y.float().sum().backward()
    torch.cuda.synchronize()
    assert (len(lib), len(generic), len(gemm), len(thin)) == expect
    assert torch.isfinite(y).all()
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


# 6. determinism: fixed reduction order, no atomics, a grid that depends on
# M and constants only
def test_bitwise_deterministic_kernel_and_layer(monkeypatch):
    monkeypatch.delenv("AMDTRAIN_PWCONV", raising=False)
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", "1")
    case = _case(777, 24, 144)
    c1, s1 = _run_kernel(case, True)
    c2, s2 = _run_kernel(case, True, nan_tail=False)
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    k = _layer_case(144, 24)
    a, b = _run_layer(k, 144, 24), _run_layer(k, 144, 24)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0]._amdtrain_bn_stats, b[0]._amdtrain_bn_stats)


def _train_two_steps():
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    torch.manual_seed(0)
    m = build_model("mobilenet_v2", num_classes=10).to(DEV) \
        .to(memory_format=torch.channels_last).train()
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    crit = CrossEntropyLoss()
    x = torch.randn(2, 3, 64, 64, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (2,), device=DEV)
    for _ in range(2):
        opt.zero_grad(set_to_none=False)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = crit(m(x), t)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_bitwise_deterministic_model(monkeypatch):
    for name in ("AMDTRAIN_CONV1X1", "AMDTRAIN_CONVSTEM", "AMDTRAIN_DWCONV",
                 "AMDTRAIN_PWCONV"):
        monkeypatch.delenv(name, raising=False)
    a, b = _train_two_steps(), _train_two_steps()
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff


# 7. host contract
def test_host_contract():
    from amdtrain import _C

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    with pytest.raises(RuntimeError):
        _C.pw_gemm(z(64, 12), z(16, 12), False)              # K % 8
    with pytest.raises(RuntimeError):
        _C.pw_gemm(z(64, 16), z(20, 16), False)              # N % 8
    with pytest.raises(RuntimeError):
        _C.pw_gemm(z(64, 16, dtype=torch.float32),
                   z(32, 16, dtype=torch.float32), False)    # dtype
    with pytest.raises(RuntimeError):
        _C.pw_gemm(z(64, 16), z(32, 24), False)              # K mismatch
    with pytest.raises(RuntimeError):
        _C.pw_gemm(z(64, 160), z(160, 160), True)            # LDS bound
    c, stats = _C.pw_gemm(z(0, 32), z(16, 32), True)         # no launch
    assert tuple(c.shape) == (0, 16) and c.dtype == torch.bfloat16
    assert stats.numel() == 0
    c, stats = _C.pw_gemm(z(0, 32), z(16, 32), False)
    assert tuple(c.shape) == (0, 16) and stats.numel() == 0
    torch.cuda.synchronize()


# 8. 64-bit offsets: M * 96 * 2 B crosses 2^32 at row 22_369_621, first on
# the C side, then on the A side
def test_offsets_past_4gib():
    from amdtrain import _C
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("needs 12 GiB of free GPU memory")
    m, edge = 22_371_000, 22_369_621
    assert edge * 96 * 2 < 2 ** 32 <= (edge + 1) * 96 * 2
    g = torch.Generator().manual_seed(64)
    b1 = (torch.randn(96, 16, generator=g) * 0.25).bfloat16()
    b2 = (torch.randn(16, 96, generator=g) * 96 ** -0.5).bfloat16()
    torch.manual_seed(64)
    a = torch.randn(m, 16, device=DEV, dtype=torch.bfloat16)
    c1 = _C.pw_gemm(a, b1.to(DEV), False)[0]
    c2 = _C.pw_gemm(c1, b2.to(DEV), False)[0]
    torch.cuda.synchronize()
    assert tuple(c1.shape) == (m, 96) and tuple(c2.shape) == (m, 16)
    starts = torch.randint(0, m - 256, (3,), generator=g).tolist()
    windows = [(0, 128), (m - 300, m), (edge - 128, edge + 128)] \
        + [(s, s + 256) for s in starts]
    for lo, hi in windows:
        ar, c1r = a[lo:hi].cpu().double(), c1[lo:hi].cpu().double()
        ref1 = ar @ b1.double().t()
        _check(f"C1[{lo}:{hi}]", c1[lo:hi], ref1,
               _c_bound(ref1, ar.abs() @ b1.double().abs().t(), 16))
        ref2 = c1r @ b2.double().t()
        _check(f"C2[{lo}:{hi}]", c2[lo:hi], ref2,
               _c_bound(ref2, c1r.abs() @ b2.double().abs().t(), 96))
