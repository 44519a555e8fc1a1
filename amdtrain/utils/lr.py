"""Learning-rate schedule.

Behavioral parity with the reference step decay (distributed.py:374-378):
``lr = base_lr * 0.1 ** (epoch // 30)`` applied by mutating the optimizer's
param groups in place.
"""

from __future__ import annotations


def adjust_learning_rate(optimizer, epoch: int, base_lr: float,
                         decay: float = 0.1, step: int = 30) -> float:
    """Step-decay the LR and write it into every param group; returns the LR."""
    lr = base_lr * (decay ** (epoch // step))
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def warmup_learning_rate(optimizer, epoch: int, it: int, iters_per_epoch: int,
                         base_lr: float, warmup_epochs: int) -> float:
    """Linear warm-up, evaluated per iteration: step ``it`` of ``epoch`` runs
    at ``base_lr * (k + 1) / total`` where ``k`` counts iterations from the
    start of training and ``total = warmup_epochs * iters_per_epoch``, so the
    last warm-up step runs at ``base_lr``.  After warm-up this is the step
    decay of ``adjust_learning_rate``."""
    k = epoch * iters_per_epoch + it
    total = warmup_epochs * iters_per_epoch
    if k >= total:
        return adjust_learning_rate(optimizer, epoch, base_lr)
    lr = base_lr * (k + 1) / total
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr
