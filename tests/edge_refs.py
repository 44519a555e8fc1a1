"""fp64 CPU references for the loss, accuracy and pooling edge tests
(tests/test_gpu_loss_pool_edges.py, tests/test_loss_pool_edges_cpu.py).

Every helper takes the values as stored (``x.double()`` of a bf16 / fp16 /
fp32 tensor is exact), works on the CPU and is deterministic.
"""

import torch
import torch.nn.functional as F


NEG, POS, NAN = float("-inf"), float("inf"), float("nan")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def ce_masked_batch(kind, dtype=torch.float32):
    """(logits [5,65], target [5]) on the CPU with -inf classes in rows 1
    and 3; rows 0, 2 and 4 stay plain.  5 rows are two blocks of the kernel
    (4 rows each), 65 classes give lane 0 a second value.  Kinds:
      col0        column 0 masked (the first value lane 0 sees)
      cols0_63    columns 0..63 masked: every lane's first value
      col64       a column >= 64 masked (lane 0's second value)
      all_but_t   only the label left: loss 0 and gradient 0 exactly
                  (label at 0 in row 1, at C-1 in row 3)
      target      the label itself masked: loss +inf
    """
    torch.manual_seed(1234)
    x = torch.randn(5, 65) * 3
    t = torch.tensor([0, 7, 64, 30, 12])
    if kind == "col0":
        x[1, 0] = x[3, 0] = NEG
    elif kind == "cols0_63":
        x[1, :64] = x[3, :64] = NEG
        t[1] = t[3] = 64
    elif kind == "col64":
        x[1, 64] = x[3, 64] = NEG
    elif kind == "all_but_t":
        t[1], t[3] = 0, 64
        keep = x[[1, 3], [0, 64]].clone()
        x[1] = x[3] = NEG
        x[[1, 3], [0, 64]] = keep
    elif kind == "target":
        x[1, 7] = x[3, 30] = NEG
    else:
        raise KeyError(kind)
    return x.to(dtype), t


CE_MASKED_KINDS = ["col0", "cols0_63", "col64", "all_but_t", "target"]


def rank_nonfinite_batch(dtype=torch.float32):
    """(logits [10,65], target [10]) on the CPU: small-integer logits (mass
    ties) with one non-finite pattern per row; see the comments."""
    torch.manual_seed(4321)
    x = torch.randint(-3, 4, (10, 65)).float()
    t = torch.full((10,), 20)
    x[0, 40] = POS                      # +inf off the label
    x[1, 20] = POS                      # +inf at the label ...
    x[1, 5] = x[1, 50] = POS            # ... tied with +inf on both sides
    x[2, 3] = NEG                       # -inf off the label
    x[3, 20] = NEG                      # -inf at the label ...
    x[3, 2] = x[3, 64] = NEG            # ... tied with -inf on both sides
    x[4, 64] = NAN                      # one NaN off the label, after it
    x[5, 0] = NAN                       # one NaN off the label, before it
    x[6, 20] = NAN                      # NaN at the label, alone
    x[7, 20] = x[7, 4] = x[7, 44] = NAN  # NaN at the label and both sides
    x[7, 9] = POS
    x[8] = NAN                          # all NaN
    x[9] = NAN                          # all NaN, label at index 0
    t[9] = 0
    return x.to(dtype), t


def ce_ref(logits, target, upstream=1.0):
    """Mean-reduced cross-entropy, piecewise: per-row loss [B], per-row
    logsumexp [B] and d(upstream * mean loss)/dlogits [B,C], all fp64.

    Through log_softmax, so -inf (masked) classes cost nothing and get a zero
    gradient, a -inf label gives loss +inf, and a +inf or NaN logit makes
    its own row non-finite and no other."""
    x = logits.detach().double().cpu()
    t = target.detach().cpu().long().reshape(-1, 1)
    lsm = torch.log_softmax(x, dim=1)
    loss = -lsm.gather(1, t)[:, 0]
    lse = torch.logsumexp(x, dim=1)
    onehot = torch.zeros_like(x).scatter_(1, t, 1.0)
    dlogits = (lsm.exp() - onehot) * (float(upstream) / x.size(0))
    return loss, lse, dlogits


def rank_ref(logits, target):
    """Position of the label in a stable descending sort of its row [B],
    int64: NaN first, then +inf down to -inf, equal values by lower index.
    This, not ``torch.topk`` (whose tie order is implementation-defined), is
    the contract of ``topk_ranks``."""
    order = torch.sort(logits.detach().double().cpu(), dim=1,
                       descending=True, stable=True).indices
    t = target.detach().cpu().long().reshape(-1, 1)
    return (order == t).long().argmax(dim=1)


def maxpool_ref(x, g):
    """3x3 stride-2 pad-1 max pool of x [N,C,H,W] and its input gradient for
    the output gradient g, both fp64 NCHW.  CPU rules: NaN propagates, ties
    go to the first tap in row-major window order, an all -inf window to its
    first tap inside the image."""
    xd = x.detach().double().cpu().contiguous().requires_grad_(True)
    y = F.max_pool2d(xd, 3, 2, 1)
    y.backward(g.detach().double().cpu().contiguous())
    return y.detach(), xd.grad
