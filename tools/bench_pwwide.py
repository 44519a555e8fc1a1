"""Pointwise 1x1 convs on the 8 grid: the pw8_gemm kernel (pwgemm8.hip)
against the routing from before it, which AMDTRAIN_PWWIDE=0 restores (MFMA
GEMM, generic element-gather kernel or MIOpen, see docs/KERNELS.md), on the
ten pointwise shapes of mobilenet_v2_140 off the 32 grid at 224 input.

    python tools/bench_pwwide.py [BATCH]      (default 256)

Both sides run through the same ``AmdConv2d`` layer under bf16 autocast in
one process, alternating; the environment switch alone decides the path, and
the library is set up as in ``bench.py`` (MIOPEN_FIND_MODE=FAST,
``cudnn.benchmark``).  Forward is the layer call; dgrad and wgrad are
``torch.autograd.grad`` of kept graphs in which only the input, or only the
weight, requires a gradient.  A pass whose old route raises (the MFMA GEMM's
input gradient needs out % 32 == 0) is reported as such.  wgrad is tn2_wgrad
on both sides of every layer that the old route serves in HIP: its rows show
the run-to-run spread of the session.

The kernel alone is timed through ``_C`` with either n-tile forced and
compared with the floor of 2*M*(K+N) bytes (read A, write C, bf16) at
``PEAK_TBS`` and with 2*M*K*N flop at ``PEAK_TFLOPS``."""
import os
import sys
import time
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402
from amdtrain.ops.conv import AmdConv2d  # noqa: E402

# (Cin, Cout, H = W) of the pw_wide_ok layers of mobilenet_v2_140 at 224
SHAPES = [(192, 48, 56), (48, 288, 56), (288, 48, 56), (288, 88, 28),
          (88, 528, 28), (528, 88, 28), (528, 136, 28), (136, 816, 14),
          (816, 136, 14), (816, 224, 14)]
PEAK_TBS = 8.0          # MI355X HBM3E, nominal
PEAK_TFLOPS = 2500.0    # MI355X dense bf16 MFMA, nominal


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
    """One routing of the layer: AMDTRAIN_PWWIDE is set around every call."""

    def __init__(self, mode, conv, x, gy):
        self.mode, self.conv, self.x, self.gy = mode, conv, x, gy
        conv.weight.requires_grad_(False)
        self.x_leaf = x.detach().requires_grad_(True)
        self.y_dx = self._call(self.x_leaf, True)
        conv.weight.requires_grad_(True)
        self.y_dw = self._call(x, True)
        self.y = self.y_dw.detach()

    def _call(self, x, grad):
        os.environ["AMDTRAIN_PWWIDE"] = self.mode
        with torch.set_grad_enabled(grad), \
                torch.autocast("cuda", dtype=torch.bfloat16):
            return self.conv(x)

    def fwd(self):
        return self._call(self.x, False)

    def dgrad(self):
        os.environ["AMDTRAIN_PWWIDE"] = self.mode
        return torch.autograd.grad(self.y_dx, self.x_leaf, self.gy,
                                   retain_graph=True)[0]

    def wgrad(self):
        os.environ["AMDTRAIN_PWWIDE"] = self.mode
        return torch.autograd.grad(self.y_dw, self.conv.weight, self.gy,
                                   retain_graph=True)[0]


def ab(new, old, name):
    """Best of three alternating rounds per side; None where a side raises."""
    fn_new, fn_old = getattr(new, name), getattr(old, name)
    try:
        fn_old()
    except RuntimeError:
        fn_old = None
    tn, to = [], []
    for _ in range(3):
        tn.append(time_fn(fn_new))
        if fn_old is not None:
            to.append(time_fn(fn_old))
    return min(tn), (min(to) if to else None)


def run(n, cin, cout, hw):
    torch.manual_seed(0)
    x = torch.randn(n, cin, hw, hw, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, cout, hw, hw, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    conv = AmdConv2d(cin, cout, 1, bias=False).cuda() \
        .to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(cout, cin, 1, 1, device="cuda")
                           * cin ** -0.5).bfloat16())
    new = Side("1", conv, x, gy)
    old = Side("0", conv, x, gy)
    m = n * hw * hw
    rel = ((new.y.float() - old.y.float()).abs().max()
           / old.y.float().abs().max()).item()
    print(f"{cin}->{cout} hw={hw} n={n} M={m}: rel|dy| {rel:.3g}", flush=True)
    nbytes = 2.0 * m * (cin + cout)     # the same for all three passes
    for name in ("fwd", "dgrad", "wgrad"):
        tn, to = ab(new, old, name)
        old_s = "raises" if to is None else \
            f"{to*1e6:8.1f} us {nbytes/to/1e12:5.2f} TB/s | x{to/tn:5.2f}"
        print(f"  {name:5s} new {tn*1e6:8.1f} us {nbytes/tn/1e12:5.2f} TB/s"
              f" | old {old_s}", flush=True)
    x2d = x.permute(0, 2, 3, 1).reshape(-1, cin)
    gy2d = gy.permute(0, 2, 3, 1).reshape(-1, cout)
    w2d = conv.weight.detach().bfloat16().reshape(cout, cin)
    wt = _C.transpose_2d(w2d)
    flop = 2.0 * m * cin * cout
    for name, a, b, st in (("fwd", x2d, w2d, True),
                           ("dgrad", gy2d, wt, False)):
        for nt in (64, 128):
            t = min(time_fn(lambda: _C.pw8_gemm(a, b, st, nt))
                    for _ in range(2))
            print(f"  kernel {name:5s} n-tile {nt:3d}: {t*1e6:8.1f} us"
                  f" {nbytes/t/1e12:5.2f} TB/s"
                  f" ({nbytes/t/1e12/PEAK_TBS:4.0%} of the byte floor's rate)"
                  f" {flop/t/1e12:6.1f} TFLOP/s"
                  f" ({flop/t/1e12/PEAK_TFLOPS:4.0%})", flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    batch = int(args[0]) if args else 256
    for cin, cout, hw in SHAPES:
        run(batch, cin, cout, hw)
    os.environ.pop("AMDTRAIN_PWWIDE", None)
