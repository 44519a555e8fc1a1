"""GPU tests for the kernels that stop issuing MFMA work on structural
zeros: the width space-to-depth stem (AMDTRAIN_STEM_S2D), the parity-class
stride-2 conv3x3 dgrad (AMDTRAIN_CONV3X3_S2PARITY) and the 64-wide conv3x3
n-tile (AMDTRAIN_CONV3X3_NT64).

The stem is checked against a float64 reference built from the same
bf16-rounded inputs; the two conv3x3 variants must reproduce the kernels
they replace value for value."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SWITCHES = ("AMDTRAIN_STEM_S2D", "AMDTRAIN_CONV3X3_S2PARITY",
            "AMDTRAIN_CONV3X3_NT64")


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available()
    from amdtrain import _C
    return _C


def _bf16r(t):
    return t.bfloat16().float()


# ---------------------------------------------------------------- stem ----

def _stem_case(n, h, w, cout):
    """bf16-representable inputs + the float64 reference (computed once per
    shape, on the CPU) with the |.|-conv scales of the error bounds."""
    g = torch.Generator().manual_seed(1000 * n + 10 * h + w + cout)
    x = _bf16r(torch.randn(n, 3, h, w, generator=g))
    wt = _bf16r(torch.randn(cout, 3, 7, 7, generator=g) * 147 ** -0.5)
    ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    gy = _bf16r(torch.randn(n, cout, ho, wo, generator=g))
    x64, w64, g64 = x.double(), wt.double(), gy.double()
    w64r = w64.clone().requires_grad_(True)
    ref = F.conv2d(x64, w64r, stride=2, padding=3)
    (dw_ref,) = torch.autograd.grad(ref, w64r, g64)
    s_fwd = F.conv2d(x64.abs(), w64.abs(), stride=2, padding=3)
    wa = w64.clone().requires_grad_(True)
    (s_w,) = torch.autograd.grad(
        F.conv2d(x64.abs(), wa, stride=2, padding=3), wa, g64.abs())
    return dict(x=x, w=wt, gy=gy, ref=ref.detach(), dw_ref=dw_ref,
                s_fwd=s_fwd, s_w=s_w, M=n * ho * wo)


_STEM_CACHE = {}


def _stem_ref(shape):
    if shape not in _STEM_CACHE:
        _STEM_CACHE[shape] = _stem_case(*shape)
    return _STEM_CACHE[shape]


def _run_stem(c):
    from amdtrain.ops.conv import conv_stem_mfma
    x = c["x"].to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    wg = c["w"].to(DEV).clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv_stem_mfma(x, wg, 2, 3)
    stats = getattr(y, "_amdtrain_bn_stats", None)
    y.backward(c["gy"].to(DEV).to(y.dtype))
    torch.cuda.synchronize()
    return (y.detach().double().cpu(), wg.grad.double().cpu(),
            None if stats is None else stats.double().cpu())


def _check_stem(c, y, dw, tag):
    # one bf16 rounding of an fp32 sum of at most 256 terms
    tol = 2.0 ** -8 * c["ref"].abs() + 2.0 ** -16 * c["s_fwd"]
    err = (y - c["ref"]).abs()
    print(f"{tag}: fwd max err/tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), (tag, (err / tol).max().item())
    tol_w = (c["M"] + 256) * 2.0 ** -24 * c["s_w"]
    err_w = (dw - c["dw_ref"]).abs()
    print(f"{tag}: wgrad max err/tol "
          f"{(err_w / tol_w.clamp_min(1e-300)).max().item():.3f}")
    assert (err_w <= tol_w).all(), \
        (tag, (err_w / tol_w.clamp_min(1e-300)).max().item())
    return tol


@pytest.mark.parametrize("shape", [(2, 32, 32, 64), (1, 20, 28, 64),
                                   (3, 18, 18, 16)])
def test_stem_s2d_vs_float64(shape, monkeypatch):
    """Forward, weight gradient and collapsed statistics partials of the
    space-to-depth stem, and the same forward / weight-gradient bounds for
    the 49-tap path it replaces.  (3,18,18,16) masks 48 of the 64 tile
    columns; (1,20,28,64) has M = 140, a 12-row tail tile."""
    _ext()
    c = _stem_ref(shape)
    monkeypatch.setenv("AMDTRAIN_STEM_S2D", "1")
    y, dw, stats = _run_stem(c)
    tol = _check_stem(c, y, dw, "s2d")
    assert stats is not None, "s2d stem must emit BN-statistics partials"
    cout = shape[3]
    nbm = (c["M"] + 127) // 128
    assert stats.shape == (nbm, 2 * cout)
    got = stats.sum(0)
    ref = c["ref"]
    # the forward bound applied per element of each sum
    tol_s1 = tol.sum((0, 2, 3))
    tol_s2 = (2 * ref.abs() * tol + tol * tol).sum((0, 2, 3))
    e1 = (got[:cout] - ref.sum((0, 2, 3))).abs()
    e2 = (got[cout:] - (ref * ref).sum((0, 2, 3))).abs()
    print(f"stats: sum err/tol {(e1 / tol_s1).max().item():.4f}  "
          f"sumsq err/tol {(e2 / tol_s2).max().item():.4f}")
    assert (e1 <= tol_s1).all(), (e1 / tol_s1).max().item()
    assert (e2 <= tol_s2).all(), (e2 / tol_s2).max().item()

    monkeypatch.setenv("AMDTRAIN_STEM_S2D", "0")
    y0, dw0, stats0 = _run_stem(c)
    _check_stem(c, y0, dw0, "49-tap")
    assert stats0 is None


def test_stem_odd_width_takes_fallback(monkeypatch):
    """Odd W has no pixel pairs: the 49-tap path runs (no statistics
    partials) and meets the same bounds."""
    _ext()
    c = _stem_ref((2, 21, 21, 64))
    monkeypatch.setenv("AMDTRAIN_STEM_S2D", "1")
    y, dw, stats = _run_stem(c)
    assert stats is None
    _check_stem(c, y, dw, "odd-W")


# ------------------------------------------------- conv3x3 variants ----

def _conv3x3_operands(n, cin, cout, hw, stride, seed):
    torch.manual_seed(seed)
    ho = (hw + 2 - 3) // stride + 1
    x2d = torch.randn(n * hw * hw, cin, device=DEV).bfloat16()
    w2d = (torch.randn(cout, 9 * cin, device=DEV) * (9 * cin) ** -0.5) \
        .bfloat16()
    gy2d = torch.randn(n * ho * ho, cout, device=DEV).bfloat16()
    return x2d, w2d, gy2d


@pytest.mark.parametrize("n,cin,cout,hw", [
    (2, 64, 64, 8),      # 32 rows per class: less than one tile
    (3, 128, 256, 12),   # 108 rows per class, two n-tiles, 8 k-steps
    (1, 32, 32, 6),
    (2, 64, 64, 29),     # odd H, W: all-taps fallback
])
def test_s2_dgrad_parity_classes_equal_all_taps(n, cin, cout, hw):
    """Parity-class tiles issue exactly the nonzero terms of the all-taps
    loop in the same order: the input gradient must be identical, on the
    128-wide and (Cin <= 64) the 64-wide n-tile.  The all-taps kernel is
    itself checked against torch in test_gpu_conv3x3.py."""
    e = _ext()
    _, w2d, gy2d = _conv3x3_operands(n, cin, cout, hw, 2, 7)
    base = e.conv3x3_dgrad(gy2d, n, hw, hw, 2, w2d, False, False, False)
    for nt64 in (False, True):
        got = e.conv3x3_dgrad(gy2d, n, hw, hw, 2, w2d, False, True, nt64)
        assert torch.equal(got, base), \
            (nt64, (got.float() - base.float()).abs().max().item())


@pytest.mark.parametrize("stride", [1, 2])
def test_nt64_tile_equals_128_tile(stride):
    """(N, C, HW) = (2, 64, 10): M = 200 / 50.  Per-element K order and
    per-block row sets do not depend on the n-tile width, so outputs and
    statistics partials must be identical."""
    e = _ext()
    n, c, hw = 2, 64, 10
    x2d, w2d, gy2d = _conv3x3_operands(n, c, c, hw, stride, 11)
    y1, s1 = e.conv3x3_fwd_stats(x2d, n, hw, hw, stride, w2d, False, True)
    y0, s0 = e.conv3x3_fwd_stats(x2d, n, hw, hw, stride, w2d, False, False)
    assert torch.equal(y1, y0)
    assert torch.equal(s1, s0)
    assert torch.equal(e.conv3x3_fwd(x2d, n, hw, hw, stride, w2d, True), y0)
    d1 = e.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d, False, False, True)
    d0 = e.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d, False, False, False)
    assert torch.equal(d1, d0)


# ------------------------------------------------------ model level ----

@pytest.mark.parametrize("arch,size", [("resnet50", 224), ("resnet18", 224)])
def test_model_step_switches_on_vs_off(arch, size, monkeypatch):
    """One training step at batch 4 with all three switches on against all
    three off.  The conv3x3 variants are value-for-value; the stem differs
    in the last bits (K grouping, BN statistics from the fp32 accumulator),
    which the forward carries into every logit, so loss and logits are
    held to the magnitude-relative bound tests/test_gpu_train.py uses for
    bf16 path comparisons (0.12 * max|ref| + 2e-3)."""
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    _ext()

    def run(on):
        for k in SWITCHES:
            monkeypatch.setenv(k, "1" if on else "0")
        torch.manual_seed(3)
        m = build_model(arch).to(DEV).to(memory_format=torch.channels_last)
        opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9)
        x = torch.randn(4, 3, size, size, device=DEV) \
            .contiguous(memory_format=torch.channels_last)
        t = torch.randint(0, 1000, (4,), device=DEV)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x)
        loss = CrossEntropyLoss()(out, t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        return loss.item(), out.detach().float()

    l1, o1 = run(True)
    l0, o0 = run(False)
    assert l1 == l1 and abs(l1) != float("inf"), l1
    assert l0 == l0 and abs(l0) != float("inf"), l0
    dl = abs(l1 - l0)
    do = (o1 - o0).abs().max().item()
    print(f"{arch}: |dloss| {dl:.3e}  max|dlogit| {do:.3e}  "
          f"max|logit| {o0.abs().max().item():.3e}")
    assert dl <= 0.12 * abs(l0) + 2e-3, (l1, l0)
    assert do <= 0.12 * o0.abs().max().item() + 2e-3, do
