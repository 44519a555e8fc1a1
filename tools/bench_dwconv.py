"""Depthwise 3x3: the stencil kernels (dwconv.hip) against the library path
that AMDTRAIN_DWCONV=miopen takes, on the ten MobileNetV2 depthwise shapes
at 224 input.

    python tools/bench_dwconv.py [BATCH]        (default 256)

Both sides run through the same ``AmdConv2d`` layer under bf16 autocast; the
environment switch alone decides the path, and the library is set up as in
``bench.py`` (MIOPEN_FIND_MODE=FAST, ``cudnn.benchmark``), so the library
column is what a training step with AMDTRAIN_DWCONV=miopen runs.  Forward is
the layer call; dgrad and wgrad are ``torch.autograd.grad`` of kept graphs in
which only the input, or only the weight, requires a gradient, so each is
one kernel family (plus, on both sides alike, the layout/cast glue around
it; the custom wgrad figure includes building dw [C,1,3,3] from the
kernel's [9,C]).
A last column times the custom kernels alone through ``_C``: at the small
late-stage shapes the layer route is bound by Python, not by the GPU.

Prints microseconds per call and the achieved GB/s against the minimum
traffic of each pass: x + y for forward, dy + dx for dgrad, dy + x for
wgrad (bf16).  Each custom result is checked against the library result
first."""
import os
import sys
import time
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402
from amdtrain.ops.conv import AmdConv2d  # noqa: E402

# (C, stride, H = W) of the depthwise layers of mobilenet_v2 at 224 input
SHAPES = [(32, 1, 112), (96, 2, 112), (144, 1, 56), (144, 2, 56),
          (192, 1, 28), (192, 2, 28), (384, 1, 14), (576, 1, 14),
          (576, 2, 14), (960, 1, 7)]


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
    """One routing of the layer: AMDTRAIN_DWCONV is set around every call.
    Two graphs are kept, one in which only the input requires a gradient and
    one in which only the weight does, so that a backward pass is the input
    gradient alone or the weight gradient alone on either path."""

    def __init__(self, mode, conv, x, gy):
        self.mode, self.conv, self.x, self.gy = mode, conv, x, gy
        conv.weight.requires_grad_(False)
        self.x_leaf = x.detach().requires_grad_(True)
        self.y_dx = self._call(self.x_leaf, True)
        conv.weight.requires_grad_(True)
        self.y_dw = self._call(x, True)
        self.y = self.y_dw.detach()

    def _call(self, x, grad):
        os.environ["AMDTRAIN_DWCONV"] = self.mode
        with torch.set_grad_enabled(grad), \
                torch.autocast("cuda", dtype=torch.bfloat16):
            return self.conv(x)

    def fwd(self):
        return self._call(self.x, False)

    def dgrad(self):
        return torch.autograd.grad(self.y_dx, self.x_leaf, self.gy,
                                   retain_graph=True)[0]

    def wgrad(self):
        return torch.autograd.grad(self.y_dw, self.conv.weight, self.gy,
                                   retain_graph=True)[0]


def run(n, c, stride, hw):
    torch.manual_seed(0)
    ho = (hw + 2 - 3) // stride + 1
    x = torch.randn(n, c, hw, hw, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, c, ho, ho, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    conv = AmdConv2d(c, c, 3, stride=stride, padding=1, groups=c,
                     bias=False).cuda().to(memory_format=torch.channels_last)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(c, 1, 3, 3, device="cuda") / 3)
                          .bfloat16())
    custom = Side("custom", conv, x, gy)
    lib = Side("miopen", conv, x, gy)

    # agreement with the library before timing anything
    ey = (custom.y.float() - lib.y.float()).abs().max().item()
    ex = (custom.dgrad().float() - lib.dgrad().float()).abs().max().item()
    dwl = lib.wgrad().float()
    ew = ((custom.wgrad().float() - dwl).abs().max() / dwl.abs().max()).item()
    print(f"C={c} s={stride} hw={hw} n={n}: max|dy| {ey:.3g} max|ddx| "
          f"{ex:.3g} rel|ddw| {ew:.3g}", flush=True)
    # the bare kernels, without the autograd and layout glue of the layer
    x2d = x.permute(0, 2, 3, 1).reshape(-1, c)
    gy2d = gy.permute(0, 2, 3, 1).reshape(-1, c)
    w9 = conv.weight.detach().bfloat16().reshape(c, 9).t().contiguous()
    kernel = {
        "fwd": lambda: _C.dwconv3x3_fwd(x2d, n, hw, hw, stride, w9),
        "dgrad": lambda: _C.dwconv3x3_dgrad(gy2d, n, hw, hw, stride, w9),
        "wgrad": lambda: _C.dwconv3x3_wgrad(gy2d, x2d, n, hw, hw, stride),
    }
    nbytes = 2.0 * (x.numel() + gy.numel())   # the same for all three passes
    for name in ("fwd", "dgrad", "wgrad"):
        tc = best(getattr(custom, name))
        tl = best(getattr(lib, name))
        tk = best(kernel[name])
        print(f"  {name:5s} custom {tc*1e6:8.1f} us {nbytes/tc/1e9:7.0f} GB/s"
              f" | library {tl*1e6:8.1f} us {nbytes/tl/1e9:7.0f} GB/s"
              f" | x{tl/tc:5.2f} | kernel alone {tk*1e6:8.1f} us"
              f" {nbytes/tk/1e9:7.0f} GB/s", flush=True)


if __name__ == "__main__":
    torch.backends.cudnn.benchmark = True
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    for c, stride, hw in SHAPES:
        run(batch, c, stride, hw)
    os.environ.pop("AMDTRAIN_DWCONV", None)
