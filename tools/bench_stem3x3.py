"""3 -> Cout 3x3 stride-2 RGB stem: the direct kernels of stem3x3.hip
(AMDTRAIN_STEM3X3=all) against the routing from before them (=0: the generic
implicit GEMM with its channel-pad op for Cout % 16 == 0, MIOpen otherwise),
at 224 input.

    python tools/bench_stem3x3.py [BATCH] [COUT ...]   (default 256, 32 24)

Both sides run through the same ``AmdConv2d`` layer under bf16 autocast in
one process, alternating; the environment switch alone decides the path, and
the library is set up as in ``bench.py`` (MIOPEN_FIND_MODE=FAST,
``cudnn.benchmark``).  Forward is the layer call with the BN-statistics
partials off, fwd+stats with them on (only the new route has them); wgrad is
``torch.autograd.grad`` of a kept graph in which only the weight requires a
gradient.  The kernels alone are timed through ``_C`` and compared with the
least traffic, x once and y (or dY) once, at ``PEAK_TBS``."""
import os
import sys
import time
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402
from amdtrain.ops.conv import AmdConv2d  # noqa: E402

HW = 224
PEAK_TBS = 8.0          # MI355X HBM3E, nominal


def time_fn(fn, iters=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


class Side:
    """One routing of the layer: the switches are set around every call."""

    def __init__(self, mode, conv, x, gy):
        self.mode, self.conv, self.x, self.gy = mode, conv, x, gy
        self.y_dw = self._call("1", True)
        self.y = self.y_dw.detach()

    def _call(self, stats, grad):
        os.environ["AMDTRAIN_STEM3X3"] = self.mode
        os.environ["AMDTRAIN_FUSE_BNSTATS"] = stats
        with torch.set_grad_enabled(grad), \
                torch.autocast("cuda", dtype=torch.bfloat16):
            return self.conv(self.x)

    def fwd(self):
        return self._call("0", False)

    def fwd_stats(self):
        return self._call("1", False)

    def wgrad(self):
        os.environ["AMDTRAIN_STEM3X3"] = self.mode
        return torch.autograd.grad(self.y_dw, self.conv.weight, self.gy,
                                   retain_graph=True)[0]


def run(n, cout):
    torch.manual_seed(0)
    x = torch.randn(n, 3, HW, HW, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, cout, HW // 2, HW // 2, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    conv = AmdConv2d(3, cout, 3, 2, 1, bias=False).cuda() \
        .to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(cout, 3, 3, 3, device="cuda")
                           * 27 ** -0.5).bfloat16())
    new, old = Side("all", conv, x, gy), Side("0", conv, x, gy)
    m = n * (HW // 2) ** 2
    rel = ((new.y.float() - old.y.float()).abs().max()
           / old.y.float().abs().max()).item()
    nbytes = 6.0 * n * HW * HW + 2.0 * m * cout
    print(f"3->{cout} hw={HW} n={n} M={m}: rel|dy| {rel:.3g}, least traffic "
          f"{nbytes/1e6:.0f} MB", flush=True)
    for name in ("fwd", "fwd_stats", "wgrad"):
        tn, to = [], []
        for _ in range(3):                       # alternating rounds
            tn.append(time_fn(getattr(new, name)))
            to.append(time_fn(getattr(old, name)))
        tn, to = min(tn), min(to)
        print(f"  {name:9s} new {tn*1e6:8.1f} us {nbytes/tn/1e12:5.2f} TB/s"
              f" | old {to*1e6:8.1f} us {nbytes/to/1e12:5.2f} TB/s"
              f" | x{to/tn:5.2f}", flush=True)
    x4 = x.permute(0, 2, 3, 1)
    gy2d = gy.permute(0, 2, 3, 1).reshape(m, cout)
    w = conv.weight.detach().bfloat16()
    for name, fn in (("fwd", lambda: _C.stem3x3_fwd(x4, w, False)),
                     ("fwd_stats", lambda: _C.stem3x3_fwd(x4, w, True)),
                     ("wgrad", lambda: _C.stem3x3_wgrad(gy2d, x4))):
        t = min(time_fn(fn) for _ in range(2))
        print(f"  kernel {name:9s}: {t*1e6:8.1f} us {nbytes/t/1e12:5.2f} TB/s"
              f" ({nbytes/t/1e12/PEAK_TBS:4.0%} of the byte floor's rate)",
              flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True
    args = [int(a) for a in sys.argv[1:]]
    for cout in args[1:] or [32, 24]:
        run(args[0] if args else 256, cout)
    os.environ.pop("AMDTRAIN_STEM3X3", None)
    os.environ.pop("AMDTRAIN_FUSE_BNSTATS", None)
