"""Entry-level timing of the any-C BN kernels (batchnorm_anyc.h) against the
power-of-two ones at neighbouring shapes.

    python tools/bench_bn_anyc.py

Times whole extension entries (BN+ReLU, bf16) with device events around 50
back-to-back calls, median of 5 rounds: fwd_eval (finalize + apply),
fwd_train (reduce + collapse + finalize + apply) and bwd (reduce + collapse +
finalize + apply).  GB/s counts the reads and writes of the activation-sized
tensors only.  The shapes are mobilenet_v2 layer sizes at batch 256 next to
the nearest power of two; each pair is measured twice, alternating."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402

DEV = "cuda"
SHAPES = [((256, 24, 56, 56), (256, 32, 56, 56)),      # gpr 3: 85 phases
          ((256, 144, 56, 56), (256, 128, 56, 56)),    # gpr 18
          ((256, 960, 7, 7), (256, 1024, 7, 7)),       # gpr 120
          ((256, 1280, 7, 7), (256, 1024, 7, 7))]      # gpr 160: 96 idle lanes
ITERS, ROUNDS = 50, 5


def make(shape):
    n, c, h, w = shape
    x = torch.randn(shape, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    go = torch.randn(shape, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    wt = torch.rand(c, device=DEV) + 0.5
    b = torch.rand(c, device=DEV)
    rm = torch.zeros(c, device=DEV)
    rv = torch.ones(c, device=DEV)
    return x, go, wt, b, rm, rv


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / ITERS * 1e-3)
    res.sort()
    return res[len(res) // 2], res[0], res[-1]


def bench(shape):
    x, go, wt, b, rm, rv = make(shape)
    nbytes = x.numel() * 2
    y, mean, invstd, scale, shift, _ = _C.batch_norm_fwd_train(x, wt, b, rm, rv, 0.1, 1e-5, True, None)
    out = {}
    # passes: eval apply 1r+1w; train fwd reduce 1r + apply 1r+1w; bwd reduce 2r + apply 2r+1w
    for name, passes, fn in [
        ("fwd_eval_apply", 2, lambda: _C.batch_norm_fwd_eval(x, wt, b, rm, rv, 1e-5, True, None)),
        ("fwd_train", 3, lambda: _C.batch_norm_fwd_train(x, wt, b, rm, rv, 0.1, 1e-5, True, None)),
        ("bwd", 5, lambda: _C.batch_norm_bwd(x, go, None, wt, mean, invstd, True, False, scale, shift)),
    ]:
        med, lo, hi = timed(fn)
        out[name] = dict(us=med * 1e6, us_min=lo * 1e6, us_max=hi * 1e6,
                         GBps=passes * nbytes / med / 1e9)
    return out


res = {}
for anyc, pow2 in SHAPES:
    for _ in range(2):          # alternate
        for s in (anyc, pow2):
            r = bench(s)
            res.setdefault(str(s), []).append(r)
for k, v in res.items():
    for i, r in enumerate(v):
        print(k, i, json.dumps({n: {a: round(b, 1) for a, b in d.items()} for n, d in r.items()}))
