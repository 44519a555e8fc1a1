"""Thin pointwise (1x1) convs: the pw_gemm kernel (pwconv.hip) against the
routing from before it, which AMDTRAIN_PWCONV=0 restores (generic
element-gather kernel or MIOpen, see docs/KERNELS.md), on the seven
mobilenet_v2 pointwise layers off the 32 grid at 224 input.

    python tools/bench_pwconv.py [BATCH] [--grids]      (default 256)

Both sides run through the same ``AmdConv2d`` layer under bf16 autocast in
one process; the environment switch alone decides the path, and the library
is set up as in ``bench.py`` (MIOPEN_FIND_MODE=FAST, ``cudnn.benchmark``).
Forward is the layer call; dgrad and wgrad are ``torch.autograd.grad`` of
kept graphs in which only the input, or only the weight, requires a
gradient.  A last column times the kernel alone through ``_C`` (for wgrad
that is tn2_wgrad, which both sides of these layers share except where the
old side is MIOpen).

Prints microseconds per call and the achieved TB/s against the floor of
2*M*(K+N) bytes (read A, write C, bf16; for wgrad read dY and X), and that
as a fraction of ``PEAK_TBS``.  Each result of the new path is checked
against the old path first.  ``--grids`` also sweeps the grid cap of the
bare kernel."""
import os
import sys
import time
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402
from amdtrain.ops.conv import AmdConv2d  # noqa: E402

# (Cin, Cout, H = W) of the thin pointwise layers of mobilenet_v2 at 224
SHAPES = [(32, 16, 112), (16, 96, 112), (96, 24, 56), (24, 144, 56),
          (144, 24, 56), (144, 32, 28)]     # 24 -> 144 occurs twice
PEAK_TBS = 8.0                              # MI355X HBM3E, nominal


def time_fn(fn, iters=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def best(fn):
    return min(time_fn(fn), time_fn(fn))


class Side:
    """One routing of the layer: AMDTRAIN_PWCONV is set around every call."""

    def __init__(self, mode, conv, x, gy):
        self.mode, self.conv, self.x, self.gy = mode, conv, x, gy
        conv.weight.requires_grad_(False)
        self.x_leaf = x.detach().requires_grad_(True)
        self.y_dx = self._call(self.x_leaf, True)
        conv.weight.requires_grad_(True)
        self.y_dw = self._call(x, True)
        self.y = self.y_dw.detach()

    def _call(self, x, grad):
        os.environ["AMDTRAIN_PWCONV"] = self.mode
        with torch.set_grad_enabled(grad), \
                torch.autocast("cuda", dtype=torch.bfloat16):
            return self.conv(x)

    def fwd(self):
        return self._call(self.x, False)

    def dgrad(self):
        os.environ["AMDTRAIN_PWCONV"] = self.mode
        return torch.autograd.grad(self.y_dx, self.x_leaf, self.gy,
                                   retain_graph=True)[0]

    def wgrad(self):
        os.environ["AMDTRAIN_PWCONV"] = self.mode
        return torch.autograd.grad(self.y_dw, self.conv.weight, self.gy,
                                   retain_graph=True)[0]


def make_layer(cin, cout):
    # the model keeps 32 -> 16 off the MFMA GEMM with this class
    from amdtrain.models.mobilenet import LibraryConv2d
    cls = LibraryConv2d if (cin, cout) == (32, 16) else AmdConv2d
    return cls(cin, cout, 1, bias=False).cuda() \
        .to(memory_format=torch.channels_last)


def run(n, cin, cout, hw, grids):
    torch.manual_seed(0)
    x = torch.randn(n, cin, hw, hw, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, cout, hw, hw, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    conv = make_layer(cin, cout)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(cout, cin, 1, 1, device="cuda")
                           * cin ** -0.5).bfloat16())
    new = Side("1", conv, x, gy)
    old = Side("0", conv, x, gy)

    def rel(a, b):
        return ((a.float() - b.float()).abs().max()
                / b.float().abs().max()).item()

    m = n * hw * hw
    print(f"{cin}->{cout} hw={hw} n={n} M={m}: rel|dy| {rel(new.y, old.y):.3g}"
          f" rel|ddx| {rel(new.dgrad(), old.dgrad()):.3g}"
          f" rel|ddw| {rel(new.wgrad(), old.wgrad()):.3g}", flush=True)
    x2d = x.permute(0, 2, 3, 1).reshape(-1, cin)
    gy2d = gy.permute(0, 2, 3, 1).reshape(-1, cout)
    w2d = conv.weight.detach().bfloat16().reshape(cout, cin)
    wt = _C.transpose_2d(w2d)
    kernel = {
        "fwd": lambda: _C.pw_gemm(x2d, w2d, True),
        "dgrad": lambda: _C.pw_gemm(gy2d, wt, False),
        "wgrad": lambda: _C.tn2_wgrad(gy2d, x2d),
    }
    nbytes = 2.0 * m * (cin + cout)     # the same for all three passes
    for name in ("fwd", "dgrad", "wgrad"):
        tn = best(getattr(new, name))
        to = best(getattr(old, name))
        tk = best(kernel[name])
        print(f"  {name:5s} new {tn*1e6:8.1f} us {nbytes/tn/1e12:5.2f} TB/s"
              f" ({nbytes/tn/1e12/PEAK_TBS:4.0%})"
              f" | old {to*1e6:8.1f} us {nbytes/to/1e12:5.2f} TB/s"
              f" | x{to/tn:5.2f} | kernel alone {tk*1e6:8.1f} us"
              f" {nbytes/tk/1e12:5.2f} TB/s"
              f" ({nbytes/tk/1e12/PEAK_TBS:4.0%})", flush=True)
    if grids:
        for name, a, b, st in (("fwd", x2d, w2d, True),
                               ("dgrad", gy2d, wt, False)):
            row = [f"{g}: {best(lambda: _C.pw_gemm(a, b, st, g))*1e6:.1f}"
                   for g in (256, 512, 768, 1024, 1536, 2048, 4096)]
            print(f"  {name:5s} grid cap -> us  " + "  ".join(row),
                  flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    batch = int(args[0]) if args else 256
    for cin, cout, hw in SHAPES:
        run(batch, cin, cout, hw, "--grids" in sys.argv)
    os.environ.pop("AMDTRAIN_PWCONV", None)
