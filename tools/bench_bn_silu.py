"""BN -> SiLU: the fused any-C kernels against the route AMDTRAIN_BN_SILU=0
selects (linear BN kernels, then ``F.silu`` in each direction), on BN -> SiLU
sites of efficientnet_b0 at 224 input.

    python tools/bench_bn_silu.py [BATCH]    (default 256)

Prints microseconds per call (device events around 50 calls after 10 warm-up
calls, best of two windows) for the training forward and for forward +
backward, and the TB/s of the fused route's minimum traffic: x twice and y
once forward (reduce, apply), x and dy twice and dx once backward.  The two
routes are checked against each other before anything is timed."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain.models.resnet import FusedBatchNorm2d  # noqa: E402
from amdtrain.ops import fused  # noqa: E402

# (C, H = W): stem, the widest early expand, depthwise outputs, the head
SHAPES = [(32, 112), (96, 112), (144, 56), (240, 28), (480, 14), (672, 14),
          (1152, 7), (1280, 7)]


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


def run(n, c, side):
    torch.manual_seed(0)
    bn = FusedBatchNorm2d(c).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-1, 1)
    x = torch.randn(n, c, side, side, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.randn_like(x)

    def fwd(route):
        os.environ["AMDTRAIN_BN_SILU"] = route
        return fused.batch_norm(x, bn, silu=True)

    def both(route):
        y = fwd(route)
        return (y,) + torch.autograd.grad(y, [x, bn.weight, bn.bias], dy)

    errs = [((a.float() - b.float()).abs().max()
             / b.float().abs().max().clamp_min(1e-30)).item()
            for a, b in zip(both("1"), both("0"))]
    t = 2.0 * x.numel()  # bytes of one tensor pass
    with torch.no_grad():
        f1, f0 = time_us(lambda: fwd("1")), time_us(lambda: fwd("0"))
    b1, b0 = time_us(lambda: both("1")), time_us(lambda: both("0"))
    print(f"{side}x{side}x{c} n={n}: fwd fused {f1:7.1f} us "
          f"({3 * t / f1 / 1e6:5.2f} TB/s), composed {f0:7.1f} us | fwd+bwd "
          f"fused {b1:7.1f} us ({8 * t / b1 / 1e6:5.2f} TB/s), composed "
          f"{b0:7.1f} us, x{b0 / b1:4.2f} | max rel diff (y, dx, dw, db) "
          + " ".join(f"{e:.2g}" for e in errs), flush=True)


if __name__ == "__main__":
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    for c, side in SHAPES:
        run(batch, c, side)
    os.environ.pop("AMDTRAIN_BN_SILU", None)
