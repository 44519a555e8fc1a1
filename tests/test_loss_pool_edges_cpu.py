"""The fp64 references of tests/edge_refs.py against hand-written cases, and
the CPU fallbacks of ``cross_entropy`` / ``topk_ranks`` against those
references on the non-finite and tie cases the GPU kernels are held to in
tests/test_gpu_loss_pool_edges.py."""

import math

import pytest
import torch

from amdtrain.ops import functional as OF
from amdtrain.utils import accuracy
from edge_refs import (CE_MASKED_KINDS, DTYPES, NAN, NEG, POS, ce_masked_batch,
                       ce_ref, maxpool_ref, rank_nonfinite_batch, rank_ref)


# ---------- the helpers themselves ----------

def test_ce_ref_hand_cases():
    # two equal classes: loss ln 2, lse x + ln 2, gradient +-1/2 / B
    x = torch.tensor([[3.0, 3.0], [0.0, NEG]])
    loss, lse, d = ce_ref(x, torch.tensor([1, 0]), upstream=4.0)
    ln2 = math.log(2.0)
    assert loss.dtype == lse.dtype == d.dtype == torch.float64
    assert torch.allclose(loss, torch.tensor([ln2, 0.0], dtype=torch.float64),
                          atol=1e-15)
    assert torch.allclose(lse, torch.tensor([3 + ln2, 0.0],
                                            dtype=torch.float64), atol=1e-15)
    want = torch.tensor([[0.5, -0.5], [0.0, 0.0]], dtype=torch.float64) * 2.0
    assert torch.allclose(d, want, atol=1e-15)
    # the masked row is exact: loss 0, gradient 0
    assert loss[1] == 0 and (d[1] == 0).all()


def test_ce_ref_nonfinite_rows_stay_local():
    x = torch.tensor([[1.0, 2.0, 3.0], [POS, 0.0, 0.0], [NAN, 0.0, 0.0],
                      [NEG, 0.0, 0.0], [1.0, 2.0, 3.0]])
    loss, lse, d = ce_ref(x, torch.tensor([0, 1, 1, 0, 2]))
    assert not torch.isfinite(loss[1]) and not torch.isfinite(loss[2])
    assert loss[3] == POS and torch.isfinite(lse[3])
    assert torch.allclose(d[3], torch.tensor([-1.0, 0.5, 0.5],
                                             dtype=torch.float64) / 5)
    assert torch.isfinite(loss[[0, 4]]).all()
    assert loss[0] - loss[4] == pytest.approx(2.0, abs=1e-15)


def test_ce_ref_is_shift_invariant():
    torch.manual_seed(0)
    x = torch.randn(4, 9)
    t = torch.tensor([0, 8, 3, 3])
    a = ce_ref(x, t)
    b = ce_ref(x.double() + 1000.0, t)
    assert torch.allclose(a[0], b[0], atol=1e-12)
    assert torch.allclose(a[1] + 1000.0, b[1], atol=1e-12)
    assert torch.allclose(a[2], b[2], atol=1e-12)


def test_rank_ref_hand_cases():
    #                 0    1    2    3    4    5
    x = torch.tensor([[1.0, NAN, POS, 1.0, NEG, NAN]]).repeat(6, 1)
    # stable descending order: NaN(1) NaN(5) +inf(2) 1(0) 1(3) -inf(4)
    t = torch.arange(6)
    assert rank_ref(x, t).tolist() == [3, 0, 2, 4, 5, 1]
    allnan = torch.full((3, 4), NAN)
    assert rank_ref(allnan, torch.tensor([0, 2, 3])).tolist() == [0, 2, 3]
    ties = torch.zeros(2, 5)
    assert rank_ref(ties, torch.tensor([0, 4])).tolist() == [0, 4]


def test_maxpool_ref_tie_and_nonfinite_rules():
    # all-zero 4x4: windows at rows/cols {-1..1} and {1..3}; first
    # occurrence inside the image is (0,0), (0,1), (1,0), (1,1)
    y, dx = maxpool_ref(torch.zeros(1, 1, 4, 4), torch.ones(1, 1, 2, 2))
    want = torch.zeros(4, 4, dtype=torch.float64)
    want[:2, :2] = 1
    assert torch.equal(dx[0, 0], want) and (y == 0).all()
    # all -inf behaves the same; a NaN tap propagates to its windows
    y, dx = maxpool_ref(torch.full((1, 1, 4, 4), NEG), torch.ones(1, 1, 2, 2))
    assert (y == NEG).all() and torch.equal(dx[0, 0], want)
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 4, 4] = NAN
    y, _ = maxpool_ref(x, torch.ones(1, 1, 3, 3))
    nan = torch.zeros(3, 3, dtype=torch.bool)
    nan[2, 2] = True
    assert torch.equal(y[0, 0].isnan(), nan)


# ---------- CPU fallback of topk_ranks ----------

@pytest.mark.parametrize("C", [1, 10, 64, 65, 1000])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_topk_ranks_cpu_ties(B, C):
    torch.manual_seed(B * 1009 + C)
    x = torch.randint(-3, 4, (B, C)).float()
    for t in (torch.randint(0, C, (B,)), torch.zeros(B, dtype=torch.long),
              torch.full((B,), C - 1)):
        for dtype in DTYPES:
            got = OF.topk_ranks(x.to(dtype), t)
            assert got.dtype == torch.int32
            assert torch.equal(got.long(), rank_ref(x.to(dtype), t))


@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_ranks_cpu_nonfinite(dtype):
    x, t = rank_nonfinite_batch(dtype)
    assert torch.equal(OF.topk_ranks(x, t).long(), rank_ref(x, t))
    # layouts: sliced logits, strided and int32 labels
    wide = torch.cat([x, torch.full_like(x, POS)], dim=1)
    pairs = torch.stack([t, (t + 1) % 65], dim=1)
    assert torch.equal(OF.topk_ranks(wide[:, :65], pairs[:, 0]).long(),
                       rank_ref(x, t))
    assert torch.equal(OF.topk_ranks(x, t.int()).long(), rank_ref(x, t))


def test_accuracy_all_nan_cpu():
    # a diverged model is not 100 % top-1: only label 0 "wins" an all-NaN row
    x = torch.full((8, 10), NAN)
    t = torch.tensor([0, 1, 2, 3, 4, 5, 6, 0])
    r = rank_ref(x, t)
    counts = OF.topk_correct_counts(x, t, (1, 5))
    assert counts.tolist() == [(r < 1).sum().item(), (r < 5).sum().item()]
    assert counts.tolist() == [2.0, 6.0]
    # accuracy() on the CPU goes through torch.topk, whose order among equal
    # (here: all NaN) entries is implementation-defined, so only "a diverged
    # model is not 100 % top-1" is pinned there
    a1, _ = accuracy(x, t, topk=(1, 5))
    assert a1.item() < 100.0


# ---------- CPU fallback of cross_entropy ----------

@pytest.mark.parametrize("kind", CE_MASKED_KINDS)
def test_cross_entropy_cpu_masked(kind):
    x, t = ce_masked_batch(kind)
    loss_ref, _, d_ref = ce_ref(x, t, upstream=1024.0)
    xg = x.clone().requires_grad_(True)
    loss = OF.cross_entropy(xg, t)
    (loss * 1024).backward()
    if kind == "target":
        assert loss.item() == POS and loss_ref.mean().item() == POS
    else:
        assert loss.item() == pytest.approx(loss_ref.mean().item(), abs=1e-5)
    if kind == "all_but_t":
        assert (loss_ref[[1, 3]] == 0).all()
        assert (xg.grad[[1, 3]] == 0).all()
    assert torch.allclose(xg.grad.double(), d_ref, atol=1e-5 * 1024 / 5,
                          rtol=2.0 ** -23)


def test_cross_entropy_cpu_nonfinite_row_stays_local():
    torch.manual_seed(7)
    x = torch.randn(5, 65)
    t = torch.randint(0, 65, (5,))
    for bad in (POS, NAN):
        xb = x.clone()
        xb[2, 11] = bad
        xg = xb.requires_grad_(True)
        loss = OF.cross_entropy(xg, t)
        loss.backward()
        assert not torch.isfinite(loss)
        _, _, d_ref = ce_ref(xb, t)
        keep = [0, 1, 3, 4]
        assert torch.allclose(xg.grad[keep].double(), d_ref[keep], atol=1e-6)
