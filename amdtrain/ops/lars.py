"""Fused multi-tensor LARS (layer-wise adaptive rate scaling) for large batches.

Momentum SGD whose update of every tensor is scaled by a trust ratio of that
tensor's own norms (You, Gitman, Ginsburg 2017)::

    r  = eta * |p| / (|g| + wd * |p| + eps)   if adapt and |p| > 0 and |g| > 0
    r  = 1                                    otherwise
    u  = r * (g + wd_t * p)                   wd_t = 0 without weight decay
    b  = u (first step)  |  mu * b + u
    p -= lr * (nesterov ? u + mu * b : b)

With ``exclude_1d`` (the usual recipe) tensors with ``ndim <= 1`` (BatchNorm
scale and shift, biases) get neither adaptation nor weight decay and step as
plain momentum SGD.  On the GPU a param group is two passes of multi-tensor
HIP launches (ops/csrc/lars.hip: chunk norms, then ratio + update + folded
grad zeroing) with no host synchronisation; ``last_trust_ratios`` keeps the
ratios of the last step on the device for logging.

``step`` has the structure of ``FusedSGD.step``: the same routing, the same
``momentum_buffer`` state, and a per-tensor torch loop with the same formula
for what the kernel does not serve.
"""

from __future__ import annotations

from typing import List

import torch
from torch.optim import Optimizer

from ._ext import require_ext
from .functional import mt_same_layout


class FusedLARS(Optimizer):
    def __init__(self, params, lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, trust_coefficient: float = 0.001,
                 eps: float = 0.0, nesterov: bool = False,
                 exclude_1d: bool = True):
        if lr < 0.0:
            raise ValueError(f"invalid lr {lr}")
        if trust_coefficient <= 0.0:
            raise ValueError(f"invalid trust_coefficient {trust_coefficient}")
        if nesterov and momentum <= 0:
            raise ValueError("nesterov requires momentum > 0")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                        trust_coefficient=trust_coefficient, eps=eps,
                        nesterov=nesterov, exclude_1d=exclude_1d)
        super().__init__(params, defaults)
        # route of the param groups of the most recent step(), as in FusedSGD
        self.last_step_fused = 0
        self.last_step_loop = 0
        # trust ratios of the most recent step(), one per stepped parameter
        # in stepping order (fp32, on the parameters' device)
        self.last_trust_ratios = torch.empty(0)

    @torch.no_grad()
    def step(self, closure=None, zero_grad: bool = False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        self.last_step_fused = 0
        self.last_step_loop = 0
        ratios: List[torch.Tensor] = []
        for group in self.param_groups:
            params: List[torch.Tensor] = []
            grads: List[torch.Tensor] = []
            bufs: List[torch.Tensor] = []
            firsts: List[bool] = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                first = "momentum_buffer" not in state
                if first and group["momentum"] != 0:
                    state["momentum_buffer"] = torch.zeros_like(
                        p, memory_format=torch.preserve_format)
                params.append(p)
                grads.append(p.grad)
                bufs.append(state["momentum_buffer"] if group["momentum"] != 0
                            else p.grad)  # unused when momentum==0
                firsts.append(first)

            if not params:
                continue

            # the standard LARS exclusion: 1-D tensors neither adapt nor decay
            mask = [not group["exclude_1d"] or p.ndim > 1 for p in params]
            fused_ok = (params[0].is_cuda and require_ext() is not None
                        and all(f == firsts[0] for f in firsts)
                        and all(mt_same_layout(p, g, b)
                                for p, g, b in zip(params, grads, bufs)))
            if fused_ok:
                ratios.append(require_ext().multi_tensor_lars(
                    params, grads, bufs, mask, mask,
                    float(group["lr"]), float(group["momentum"]),
                    float(group["weight_decay"]),
                    float(group["trust_coefficient"]), float(group["eps"]),
                    bool(group["nesterov"]),
                    bool(firsts[0] and group["momentum"] != 0),
                    bool(zero_grad)))
                self.last_step_fused += 1
            else:
                ratios.append(self._step_loop(group, params, grads, firsts,
                                              mask, zero_grad))
                self.last_step_loop += 1
        if ratios:
            self.last_trust_ratios = ratios[0] if len(ratios) == 1 \
                else torch.cat(ratios)
        return loss

    def _step_loop(self, group, params, grads, firsts, mask, zero_grad):
        mu, wd, lr = group["momentum"], group["weight_decay"], group["lr"]
        eta, eps, nesterov = (group["trust_coefficient"], group["eps"],
                              group["nesterov"])
        ratios = []
        for p, g, first, on in zip(params, grads, firsts, mask):
            r = torch.ones((), dtype=torch.float32, device=p.device)
            if on:
                pn, gn = p.float().norm(), g.float().norm()
                r = torch.where((pn > 0) & (gn > 0),
                                eta * pn / (gn + wd * pn + eps), r)
                if wd != 0:
                    g = g.add(p, alpha=wd)
                g = g.mul(r.to(g.dtype))
            ratios.append(r)
            if mu != 0:
                buf = self.state[p]["momentum_buffer"]
                if first:
                    buf.copy_(g)
                else:
                    buf.mul_(mu).add_(g)
                g = g.add(buf, alpha=mu) if nesterov else buf
            p.add_(g, alpha=-lr)
            if zero_grad:
                p.grad.zero_()
        return torch.stack(ratios)
