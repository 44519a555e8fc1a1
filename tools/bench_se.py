"""Squeeze-excite: the seven kernels of se.hip on the eight SE shapes of
mobilenet_v3_large at 224 input, and the whole block forward + backward
through ``squeeze_excite`` on both routes (the kernels, and the torch
composition that AMDTRAIN_SE=0 selects).

    python tools/bench_se.py [BATCH]    (default 256)

Prints microseconds per call (device events around 50 calls after 10 warm-up
calls, best of two windows) and, for the four tensor passes, the achieved
TB/s of minimum traffic: x for squeeze, x + y for scale, dy + x for the
backward reduce, dy + x + dx for the backward apply (dy + dx when the block
has no hardswish inside).  The two routes are checked against each other
before anything is timed."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402
from amdtrain.models.mobilenet import _make_divisible  # noqa: E402
from amdtrain.ops import squeeze_excite  # noqa: E402

# (C, H = W, hardswish inside) of the SE blocks of mobilenet_v3_large
SHAPES = [(72, 28, False), (120, 28, False), (120, 28, False),
          (480, 14, True), (672, 14, True), (672, 7, True),
          (960, 7, True), (960, 7, True)]


def time_us(fn, iters=50):
    best = float("inf")
    for _ in range(2):
        for _ in range(10):
            fn()
        t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1) * 1e3 / iters)
    return best


def run(n, c, hw_side, hs):
    torch.manual_seed(0)
    cs, hw = _make_divisible(c // 4, 8), hw_side * hw_side
    pre_act = "hardswish" if hs else "none"
    x = (2 * torch.randn(n, c, hw_side, hw_side, device="cuda")).bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    dy = torch.randn_like(x)
    w1 = torch.randn(cs, c, device="cuda") / c ** 0.5
    w2 = torch.randn(c, cs, device="cuda") / cs ** 0.5
    b1, b2 = torch.zeros(cs, device="cuda"), torch.zeros(c, device="cuda")
    params = [t.requires_grad_(True) for t in (w1, b1, w2, b2)]
    xl = x.detach().requires_grad_(True)

    def block(route):
        os.environ["AMDTRAIN_SE"] = route
        y = squeeze_excite(xl, *params, pre_act)
        return (y,) + torch.autograd.grad(y, [xl] + params, dy)

    ref, out = block("0"), block("1")
    errs = [((a.float() - b.float()).abs().max()
             / b.float().abs().max().clamp_min(1e-30)).item()
            for a, b in zip(out, ref)]
    print(f"C={c} Cs={cs} hw={hw_side} n={n} {pre_act}: max rel diff to the "
          f"torch route (y, dx, dw1, db1, dw2, db2) "
          + " ".join(f"{e:.2g}" for e in errs), flush=True)

    x2d = x.permute(0, 2, 3, 1).reshape(-1, c)
    dy2d = dy.permute(0, 2, 3, 1).reshape(-1, c)
    w1d, b1d, w2d, b2d = (t.detach() for t in params)
    part = _C.se_squeeze(x2d, n, hw, hs, 0)
    s, mean, hid = _C.se_excite(part, hw, w1d, b1d, w2d, b2d)
    ds_part = _C.se_bwd_reduce(dy2d, x2d, n, hw, hs, 0)
    dz2, dz1, dm = _C.se_excite_bwd(ds_part, s, hid, w1d, w2d, hw)
    t = 2.0 * x.numel()  # bytes of one tensor pass
    kernels = [
        ("se_squeeze", t, lambda: _C.se_squeeze(x2d, n, hw, hs, 0)),
        ("se_excite", 0, lambda: _C.se_excite(part, hw, w1d, b1d, w2d, b2d)),
        ("se_scale", 2 * t, lambda: _C.se_scale(x2d, s, n, hw, hs)),
        ("se_bwd_reduce", 2 * t,
         lambda: _C.se_bwd_reduce(dy2d, x2d, n, hw, hs, 0)),
        ("se_excite_bwd", 0,
         lambda: _C.se_excite_bwd(ds_part, s, hid, w1d, w2d, hw)),
        ("se_wgrad", 0, lambda: _C.se_wgrad(dz2, dz1, mean, hid)),
        ("se_bwd_apply", (3 if hs else 2) * t,
         lambda: _C.se_bwd_apply(dy2d, x2d, s, dm, n, hw, hs)),
    ]
    total = 0.0
    for name, nbytes, fn in kernels:
        us = time_us(fn)
        total += us
        rate = f" {nbytes / us / 1e6:6.2f} TB/s" if nbytes else ""
        print(f"  {name:14s} {us:8.1f} us{rate}  (splits {part.shape[1]})",
              flush=True)
    tk, tt = time_us(lambda: block("1")), time_us(lambda: block("0"))
    print(f"  kernels summed {total:8.1f} us | block fwd+bwd: kernels "
          f"{tk:8.1f} us, torch composition {tt:8.1f} us, x{tt / tk:5.2f}",
          flush=True)


if __name__ == "__main__":
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    for c, side, hs in SHAPES:
        run(batch, c, side, hs)
    os.environ.pop("AMDTRAIN_SE", None)
