"""Cross-entropy, top-k rank, max-pool, global-average-pool and
input-normalise kernels at their edges: odd batch and class counts, three
dtypes, non-finite values, ties, non-unit upstream gradients and strided
arguments, each against the fp64 CPU references of tests/edge_refs.py.
Every case is a few thousand elements at most."""

import pytest
import torch
import torch.nn.functional as F

from edge_refs import (CE_MASKED_KINDS, DTYPES, NAN, NEG, POS, ce_masked_batch,
                       ce_ref, maxpool_ref, rank_nonfinite_batch, rank_ref)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# one ulp of the output dtype, relative (bf16 / fp16 as the kernels round
# their outputs; fp32 outputs are exact copies of the fp32 arithmetic)
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8,
       torch.float16: 2.0 ** -10}
U32 = 2.0 ** -24  # unit roundoff of the kernels' fp32 arithmetic


def _C():
    from amdtrain.ops import functional as OF
    assert OF.ext_available(), (
        "amdtrain._C must be built in-tree on the GPU box")
    from amdtrain import _C
    return _C


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


# ====================== cross-entropy ======================
#
# Loss and logsumexp are fp32 outputs for every logit dtype.  Allowance:
# 4 x the worst-row error of torch's own fp32
# F.cross_entropy(reduction="none") against ce_ref ON THE SAME INPUTS
# (computed on the CPU in _ce_tol, never from the kernel), floor 1e-5; the
# kernel uses __expf / __logf, hence the margin.  Measured on the CPU over
# B in {1, 5, 67} x C in {2, 63, 64, 65, 127, 1000, 1003}:
#   randn          8.5e-7 (fp32) 7.3e-7 (bf16) 7.2e-7 (fp16) -> floor, 1e-5
#                  (the atol of test_gpu_kernels.py::test_cross_entropy)
#   randn * 20     6.9e-6 (fp32) 3.8e-6 (bf16) 3.7e-6 (fp16) -> up to 2.8e-5
#   randn + 1000   6.8e-7 (fp32)                              -> floor, 1e-5
# The logsumexp gets half an fp32 ulp of its own value on top (U32 * |lse|):
# an fp32 output cannot sit nearer to the fp64 value than that, and at
# |lse| ~ 1007 it is 3.05e-5, which torch's own fp32 logsumexp measures too.
# The gradient gets the same allowance scaled by upstream / B plus one ulp of
# the logit dtype relative to the reference.

def _ce_tol(x_cpu, t_cpu, loss_ref, rows=None):
    own = F.cross_entropy(x_cpu.float(), t_cpu, reduction="none").double()
    if rows is not None:
        own, loss_ref = own[rows], loss_ref[rows]
    ok = torch.isfinite(loss_ref)
    err = (own - loss_ref)[ok].abs().max().item() if ok.any() else 0.0
    return max(1e-5, 4.0 * err)


def _same(a, b):
    """Equal elementwise, NaN matching NaN."""
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _close(got, ref, atol, rtol, rows=None):
    """|got - ref| <= atol + rtol * |ref| elementwise, non-finite reference
    entries equal in kind; returns the worst excess for the message."""
    got, ref = got.detach().double().cpu(), ref.double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    fin = torch.isfinite(ref)
    same = _same(got[~fin], ref[~fin])
    d = (got - ref)[fin].abs() - (atol + rtol * ref[fin].abs())
    worst = d.max().item() if d.numel() else 0.0
    return same and worst <= 0.0, worst


def _make_logits(kind, B, C, dtype, seed):
    torch.manual_seed(seed)
    x = torch.randn(B, C)
    if kind == "scaled":
        x = x * 20
    elif kind == "shifted":
        x = x + 1000
    return x.to(dtype)


def _check_ce(x_cpu, t_cpu, upstream=1.0, rows=None, x_dev=None, t_dev=None):
    """Per-row forward, per-row backward and the autograd path of one batch
    against ce_ref.  ``rows``: the rows whose reference is finite and must
    match (default all).  Returns the device results."""
    from amdtrain.ops import functional as OF
    C_ = _C()
    B = x_cpu.size(0)
    dtype = x_cpu.dtype
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    t = t_cpu.to(DEV) if t_dev is None else t_dev
    loss_ref, lse_ref, d_ref = ce_ref(x_cpu, t_cpu, upstream)
    tol = _ce_tol(x_cpu, t_cpu, loss_ref, rows)

    losses, lse, lse_lo = C_.cross_entropy_fwd(x, t)
    assert losses.dtype == lse.dtype == lse_lo.dtype == torch.float32
    ok, w = _close(losses, loss_ref, tol, 0.0, rows)
    print(f"ce loss tol {tol:.3g} excess {w:.3g}")
    assert ok, ("loss", tol, w)
    ok, w = _close(lse, lse_ref, tol, U32, rows)
    print(f"ce lse excess {w:.3g}")
    assert ok, ("lse", tol, w)

    up = torch.tensor([upstream], device=DEV)
    g = C_.cross_entropy_bwd(x, t, lse, lse_lo, up)
    assert g.dtype == dtype and g.shape == x.shape and g.is_contiguous()
    ok, w = _close(g, d_ref, tol * abs(upstream) / B, ULP[dtype], rows)
    print(f"ce dlogits excess {w:.3g}")
    assert ok, ("dlogits", tol, w)

    xg = x.detach().clone().requires_grad_(True)
    if x_dev is not None:  # keep the caller's layout in the autograd path
        xg = x_dev.detach().requires_grad_(True)
    loss = OF.cross_entropy(xg, t)
    (loss * upstream).backward()
    assert _same(xg.grad, g)
    if rows is None:
        mean_ref = loss_ref.mean().item()
        if loss_ref.isfinite().all():
            # mean of B fp32 values: B * 2^-24 relative on top
            assert abs(loss.item() - mean_ref) <= \
                tol + B * U32 * loss_ref.abs().mean().item(), \
                (loss.item(), mean_ref)
        else:
            assert loss.item() == mean_ref or (
                loss.isnan().item() and mean_ref != mean_ref)
    return losses, lse, g


CE_SHAPES = [(1, 1), (5, 1), (1, 2), (5, 63), (67, 64), (5, 65), (67, 127),
             (5, 1000), (1, 1003), (67, 1003)]


@pytest.mark.parametrize("kind", ["randn", "scaled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,C", CE_SHAPES)
def test_ce_shapes(B, C, dtype, kind):
    x = _make_logits(kind, B, C, dtype, 100 * B + C)
    t = torch.randint(0, C, (B,))
    losses, _, g = _check_ce(x, t)
    if C == 1:
        assert (losses == 0).all() and (g == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("C", [2, 64, 65, 1003])
def test_ce_target_first_and_last(C, dtype):
    x = _make_logits("scaled", 5, C, dtype, 7 + C)
    _check_ce(x, torch.zeros(5, dtype=torch.long))
    _check_ce(x, torch.full((5,), C - 1))


# Shift invariance, fp32 logits of randn + 1000 (a naive softmax overflows).
# One fp32 logsumexp is off by half an ulp of |lse| ~ 1007 here (3.05e-5),
# and a loss formed as fl32(lse) - x[t] or a softmax formed as
# exp(x - fl32(lse)) inherits that: measured on an MI355X before the
# logsumexp was saved as an fp32 pair, the loss missed by 2.92e-5 at (5, 2),
# 3.06e-5 at (67, 65) and 3.05e-5 at (67, 1003) against the 1e-5 bound, and
# the gradient at (5, 2), where p ~ 0.5, by 3.6e-6 against 2e-6 plus an ulp.
_SHIFT = {}


def _shifted(B, C):
    if (B, C) not in _SHIFT:
        C_ = _C()
        x = _make_logits("shifted", B, C, torch.float32, 31 * B + C)
        t = torch.randint(0, C, (B,))
        ref = ce_ref(x, t)
        losses, lse, lse_lo = C_.cross_entropy_fwd(x.to(DEV), t.to(DEV))
        g = C_.cross_entropy_bwd(x.to(DEV), t.to(DEV), lse, lse_lo,
                                 torch.ones(1, device=DEV))
        _SHIFT[(B, C)] = (ref, _ce_tol(x, t, ref[0]), losses, lse, g, lse_lo)
    return _SHIFT[(B, C)]


SHIFT_SHAPES = [(5, 2), (67, 65), (67, 1003)]


@pytest.mark.parametrize("B,C", SHIFT_SHAPES)
def test_ce_shifted_lse(B, C):
    ref, tol, _, lse, _, lse_lo = _shifted(B, C)
    ok, w = _close(lse, ref[1], tol, U32)
    print(f"shifted lse tol {tol:.3g} excess {w:.3g}")
    assert ok, (tol, w)
    # the pair carries what the single fp32 cannot
    ok, w = _close(lse.double() + lse_lo.double(), ref[1], tol, 0.0)
    print(f"shifted lse pair excess {w:.3g}")
    assert ok, (tol, w)


@pytest.mark.parametrize("B,C", SHIFT_SHAPES)
def test_ce_shifted_loss(B, C):
    ref, tol, losses = _shifted(B, C)[:3]
    ok, w = _close(losses, ref[0], tol, 0.0)
    print(f"shifted loss tol {tol:.3g} excess {w:.3g}")
    assert ok, (tol, w)


@pytest.mark.parametrize("B,C", SHIFT_SHAPES)
def test_ce_shifted_dlogits(B, C):
    ref, tol, _, _, g, _ = _shifted(B, C)
    ok, w = _close(g, ref[2], tol / B, ULP[torch.float32])
    print(f"shifted dlogits tol {tol / B:.3g} excess {w:.3g}")
    assert ok, (tol, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("kind", CE_MASKED_KINDS)
def test_ce_masked_classes(kind, dtype):
    x, t = ce_masked_batch(kind, dtype)
    losses, lse, g = _check_ce(x, t, upstream=1024.0)
    assert torch.isfinite(lse).all()
    if kind == "all_but_t":
        assert (losses[[1, 3]] == 0).all() and (g[[1, 3]] == 0).all()
    if kind == "target":
        assert (losses[[1, 3]] == POS).all()
        assert torch.isfinite(losses[[0, 2, 4]]).all()


@pytest.mark.parametrize("bad", [POS, NAN], ids=["posinf", "nan"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ce_nonfinite_row_stays_local(dtype, bad):
    x = _make_logits("randn", 5, 65, dtype, 77)
    t = torch.randint(0, 65, (5,))
    for col in (0, 64):
        xb = x.clone()
        xb[2, col] = bad
        losses, _, _ = _check_ce(xb, t, rows=[0, 1, 3, 4])
        assert not torch.isfinite(losses[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ce_upstream_gradient(dtype):
    from amdtrain.ops import functional as OF
    _C()
    x = _make_logits("scaled", 67, 127, dtype, 5)
    t = torch.randint(0, 127, (67,))
    _check_ce(x, t, upstream=1024.0)
    xg = x.to(DEV).requires_grad_(True)
    (OF.cross_entropy(xg, t.to(DEV)) * 0.0).backward()
    assert torch.equal(xg.grad, torch.zeros_like(xg))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ce_strided_arguments(dtype):
    B, C = 67, 65
    x = _make_logits("randn", B, C, dtype, 9)
    torch.manual_seed(10)
    t = torch.randint(0, C, (B,))
    other = (t + 1 + torch.randint(0, C - 1, (B,))) % C  # valid, never == t
    wide = torch.cat([x, torch.full((B, 7), 50.0, dtype=dtype)], 1).to(DEV)
    pairs = torch.stack([t, other], 1).to(DEV)
    assert not wide[:, :C].is_contiguous()
    assert not pairs[:, 0].is_contiguous()
    _check_ce(x, t, t_dev=pairs[:, 0])
    _check_ce(x, t, x_dev=wide[:, :C])
    _check_ce(x, t, upstream=3.0, x_dev=wide[:, :C], t_dev=pairs[:, 0])


def test_ce_rejects_wrong_targets():
    from amdtrain.ops import functional as OF
    C_ = _C()
    x = torch.randn(5, 10, device=DEV)
    t = torch.randint(0, 10, (5,), device=DEV)
    _, lse, lo = C_.cross_entropy_fwd(x, t)
    one = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match="int64"):
        C_.cross_entropy_fwd(x, t.int())
    with pytest.raises(RuntimeError, match="int64"):
        C_.cross_entropy_bwd(x, t.int(), lse, lo, one)
    with pytest.raises(RuntimeError, match="int64"):
        OF.cross_entropy(x, t.int())
    with pytest.raises(RuntimeError, match="target is on"):
        C_.cross_entropy_fwd(x, t.cpu())
    with pytest.raises(RuntimeError, match="target is on"):
        C_.cross_entropy_bwd(x, t.cpu(), lse, lo, one)
    with pytest.raises(RuntimeError, match=r"\[B\]"):
        C_.cross_entropy_fwd(x, t[:4])


# ====================== top-k ranks ======================

def _check_ranks(x_cpu, t_cpu, x_dev=None, t_dev=None):
    from amdtrain.ops import functional as OF
    _C()
    x = x_cpu.to(DEV) if x_dev is None else x_dev
    t = t_cpu.to(DEV) if t_dev is None else t_dev
    got = OF.topk_ranks(x, t)
    assert got.dtype == torch.int32
    want = rank_ref(x_cpu, t_cpu)
    assert torch.equal(got.cpu().long(), want), (got.cpu(), want)


@pytest.mark.parametrize("C", [1, 10, 64, 65, 1000])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_ranks_mass_ties(B, C):
    torch.manual_seed(B * 1009 + C)
    x = torch.randint(-3, 4, (B, C)).float()
    t = torch.randint(0, C, (B,))
    for dtype in DTYPES:
        _check_ranks(x.to(dtype), t)
    _check_ranks(x, torch.zeros(B, dtype=torch.long))
    _check_ranks(x, torch.full((B,), C - 1))


@pytest.mark.parametrize("B,C", [(5, 65), (67, 1000)])
def test_ranks_bf16_randn(B, C):
    torch.manual_seed(B + C)
    x = torch.randn(B, C).bfloat16()  # 8-bit mantissa: ties among 1000
    _check_ranks(x, torch.randint(0, C, (B,)))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_ranks_nonfinite(dtype):
    x, t = rank_nonfinite_batch(dtype)
    _check_ranks(x, t)


def test_ranks_strided_arguments():
    x, t = rank_nonfinite_batch(torch.bfloat16)
    wide = torch.cat([x, torch.full_like(x, POS)], dim=1).to(DEV)
    pairs = torch.stack([t, (t + 1) % 65], dim=1).to(DEV)
    _check_ranks(x, t, x_dev=wide[:, :65])
    _check_ranks(x, t, t_dev=pairs[:, 0])
    _check_ranks(x, t, t_dev=t.int().to(DEV))
    _check_ranks(x, t, x_dev=wide[:, :65], t_dev=pairs.int()[:, 0])


def test_accuracy_all_nan_is_not_perfect():
    from amdtrain.utils import accuracy
    _C()
    x = torch.full((8, 10), NAN)
    t = torch.tensor([0, 1, 2, 3, 4, 5, 6, 0])
    r = rank_ref(x, t)
    a1, a5 = accuracy(x.to(DEV), t.to(DEV), topk=(1, 5))
    assert a1.item() == 100.0 * (r < 1).sum().item() / 8 == 25.0
    assert a5.item() == 100.0 * (r < 5).sum().item() / 8 == 75.0


# ====================== max pool 3x3 / s2 / p1 ======================

def _pool(x_cpu, g_cpu):
    from amdtrain.ops import fused as OFU
    _C()
    xg = _nhwc(x_cpu.to(DEV)).requires_grad_(True)
    y = OFU.max_pool_3x3_s2(xg)
    y.backward(_nhwc(g_cpu.to(DEV)))
    return y.detach().cpu(), xg.grad.cpu()


def _pool_case(N, C, H, W, dtype, seed):
    torch.manual_seed(seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randint(-2, 3, (N, C, H, W)).to(dtype)  # ties decide routing
    g = (torch.randint(-8, 9, (N, C, Ho, Wo)) / 8).to(dtype)  # exact sums
    return x, g


def _packs(dtype):
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    return vec, 3 * vec


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (7, 9), (8, 8), (15, 15)])
def test_maxpool_ties_exact(H, W, dtype):
    for N in (1, 3):
        for C in _packs(dtype):
            x, g = _pool_case(N, C, H, W, dtype, 1000 * H + 10 * W + N + C)
            y, dx = _pool(x, g)
            y_ref, dx_ref = maxpool_ref(x, g)
            assert torch.equal(y, y_ref.to(dtype)), (N, C)
            assert torch.equal(dx, dx_ref.to(dtype)), (N, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_maxpool_propagates_nan(dtype):
    N, C, H, W = 3, _packs(dtype)[1], 9, 9
    x, g = _pool_case(N, C, H, W, dtype, 99)
    # one NaN per image, interior: in 1, 2 and 4 windows
    for n, (c, h, w) in enumerate([(0, 4, 4), (1, 3, 4), (C - 1, 3, 5)]):
        x[n, c, h, w] = NAN
    y, dx = _pool(x, g)
    y_ref, dx_ref = maxpool_ref(x, g)
    ynan = y_ref.isnan()
    assert ynan.sum().item() == 1 + 2 + 4
    assert torch.equal(y.isnan(), ynan)
    assert torch.equal(y[~ynan], y_ref.to(dtype)[~ynan])
    # inputs that lie in a NaN-holding window: which NaN tap gets the
    # gradient is not pinned, so dx is compared everywhere else
    skip = torch.zeros(N, C, H, W, dtype=torch.bool)
    for n, c, ho, wo in ynan.nonzero().tolist():
        skip[n, c, max(0, 2 * ho - 1):2 * ho + 2,
             max(0, 2 * wo - 1):2 * wo + 2] = True
    assert 0 < skip.float().mean().item() <= 0.05
    assert torch.equal(dx[~skip], dx_ref.to(dtype)[~skip])
    # and the gradient of a NaN window is not lost: it lands inside it
    assert torch.equal(dx.double().sum((2, 3)), dx_ref.sum((2, 3)))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (8, 8)])
def test_maxpool_all_neginf_channel(H, W, dtype):
    C = _packs(dtype)[1]
    x, g = _pool_case(3, C, H, W, dtype, 5 + H)
    x[:, 1] = NEG
    x[1, C - 1] = NEG
    y, dx = _pool(x, g)
    y_ref, dx_ref = maxpool_ref(x, g)
    assert (y[:, 1] == NEG).all()
    assert torch.equal(y, y_ref.to(dtype))
    assert torch.equal(dx, dx_ref.to(dtype))


def test_maxpool_rejects_partial_packs():
    C_ = _C()
    for C in (12, 4):
        x = _nhwc(torch.zeros(1, C, 4, 4, device=DEV, dtype=torch.bfloat16))
        g = _nhwc(torch.zeros(1, C, 2, 2, device=DEV, dtype=torch.bfloat16))
        idx = _nhwc(torch.zeros(1, C, 2, 2, device=DEV, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="multiple of 8"):
            C_.max_pool_3x3_s2_fwd(x)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            C_.max_pool_3x3_s2_bwd(g, idx, 4, 4)


# ====================== global average pool ======================
#
# y = T(fp32 sum * fp32(1/HW)).  Allowance: one ulp of the output dtype
# relative to the reference, plus the recursive fp32 sum's bound
# HW * 2^-24 relative to mean|x| (the sum of |x| over HW; equal to |y| when
# the signs agree), which also covers the rounded 1/HW and the product.

def _gap_check(x_cpu, g_cpu):
    from amdtrain.ops import fused as OFU
    _C()
    dtype = x_cpu.dtype
    HW = x_cpu.size(2) * x_cpu.size(3)
    xg = _nhwc(x_cpu.to(DEV)).requires_grad_(True)
    y = OFU.global_avg_pool(xg)
    assert y.shape == (x_cpu.size(0), x_cpu.size(1), 1, 1) and y.dtype == dtype
    y.backward(g_cpu.to(DEV))
    xd = x_cpu.double()
    y_ref = xd.mean((2, 3), keepdim=True)
    acc = (HW + 2) * U32 * xd.abs().mean((2, 3), keepdim=True)
    err = (y.detach().cpu().double() - y_ref).abs()
    assert (err <= ULP[dtype] * y_ref.abs() + acc).all(), err.max().item()
    if HW == 1:
        assert torch.equal(y.detach().cpu(), x_cpu)
    dx_ref = (g_cpu.double() / HW).expand_as(xd)
    err = (xg.grad.cpu().double() - dx_ref).abs()
    assert (err <= (ULP[dtype] + 2 * U32) * dx_ref.abs()).all(), \
        err.max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (7, 7), (12, 12)])
def test_gap_edges(H, W, dtype):
    for N in (1, 3):
        for C in _packs(dtype):
            torch.manual_seed(H * 100 + N * 10 + C)
            x = (torch.randn(N, C, H, W) * 3 + 1).to(dtype)
            g = (torch.randint(1, 9, (N, C, 1, 1)) / 8).to(dtype)
            _gap_check(x, g)


@pytest.mark.parametrize("C", [12, 4])
def test_gap_partial_packs(C):
    # bf16 packs hold 8 channels: C = 12 would leave channels 8..11
    # unwritten, C = 4 is an empty grid.  The op answers through torch, the
    # kernels' entry points refuse.
    C_ = _C()
    torch.manual_seed(C)
    x = (torch.randn(3, C, 7, 7) * 3 + 1).bfloat16()
    g = (torch.randint(1, 9, (3, C, 1, 1)) / 8).bfloat16()
    _gap_check(x, g)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C_.global_avg_pool_fwd(_nhwc(x.to(DEV)))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C_.global_avg_pool_bwd(g.to(DEV), 7, 7)


# ====================== normalize_u8 ======================
#
# y = T((fp32(x) - fp32(mean)) * fp32(1 / fp32(std))): four fp32 roundings
# (mean, difference, reciprocal, product), each at most 2^-24 of 255 / std,
# then one rounding to T.

@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", [(1, 3, 3, 5), (2, 3, 5, 7)])
def test_normalize_u8_edges(shape, layout):
    # (1,3,3,5): 15 pixels, the tail loop alone; (2,3,5,7): 4 groups + 6
    from amdtrain.ops import functional as OF
    _C()
    torch.manual_seed(sum(shape))
    x = torch.randint(0, 256, shape, dtype=torch.uint8)
    x[0, :, 0, 0] = 0
    x[0, :, 0, 1] = 255
    mean, std = (10.5, 127.25, 200.0), (3.0, 64.5, 0.7)
    xd = x.to(DEV)
    xd = _nhwc(xd) if layout == "nhwc" else xd.contiguous()
    stats = [({"mean": mean, "std": std}, mean, std),
             ({}, OF.IMAGENET_MEAN_255, OF.IMAGENET_STD_255)]
    for dtype in DTYPES:
        for kw, mean_, std_ in stats:
            dm = torch.tensor(mean_, dtype=torch.float64).reshape(1, 3, 1, 1)
            sd = torch.tensor(std_, dtype=torch.float64).reshape(1, 3, 1, 1)
            r = (x.double() - dm) / sd
            y = OF.normalize_u8(xd, dtype=dtype, **kw)
            assert y.dtype == dtype and y.shape == x.shape
            assert y.is_contiguous(memory_format=torch.channels_last)
            err = (y.cpu().double() - r).abs()
            bound = ULP[dtype] * r.abs() + 4 * U32 * 255.0 / sd
            assert (err <= bound).all(), (dtype, (err - bound).max().item())
