"""conv3x3 forward / dgrad times on layer2-4 shapes, the forward
refchecked vs F.conv2d.

``--dgrad-split [B]`` instead times the dgrad (and the layer-1 forward) of
every ResNet-50 conv3x3 site at batch B, stride 1 and stride 2 apart, with
the parity-class tiles / the 64-wide n-tile switched off and on."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from amdtrain import _C  # noqa: E402


def time_fn(fn, iters=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    import time
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def run(n, cin, cout, hw, stride=1):
    torch.manual_seed(0)
    x = torch.randn(n, cin, hw, hw, device="cuda") \
        .contiguous(memory_format=torch.channels_last).bfloat16()
    w = (torch.randn(cout, cin, 3, 3, device="cuda") * (9 * cin) ** -0.5) \
        .bfloat16()
    x2d = x.permute(0, 2, 3, 1).reshape(-1, cin)
    w2d = w.contiguous(memory_format=torch.channels_last) \
        .permute(0, 2, 3, 1).reshape(cout, 9 * cin)
    ho = (hw + 2 - 3) // stride + 1

    # fwd refcheck
    ref = F.conv2d(x[:1].float(), w.float(), stride=stride, padding=1)
    y = _C.conv3x3_fwd(x2d, n, hw, hw, stride, w2d) \
        .view(n, ho, ho, cout).permute(0, 3, 1, 2)[:1].float()
    err = (y - ref).abs().max().item()
    print(f"  fwd: err {err:.4f} {'OK' if err < 0.5 else 'FAIL'}")
    flops = 2.0 * n * ho * ho * cout * 9 * cin
    t = time_fn(lambda: _C.conv3x3_fwd(x2d, n, hw, hw, stride, w2d))
    print(f"fwd n={n} c={cin}->{cout} hw={hw} s={stride}: "
          f"{t*1e6:7.1f} us ({flops/t/1e12:6.1f} TF)", flush=True)
    gy2d = torch.randn(n * ho * ho, cout, device="cuda").bfloat16()
    t = time_fn(lambda: _C.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d))
    print(f"dgrad: {t*1e6:7.1f} us ({flops/t/1e12:6.1f} TF)", flush=True)


def dgrad_split(n):
    """Per-shape dgrad times: (sites per step, cin, cout, hw, stride)."""
    tot = {"off": 0.0, "on": 0.0}
    for cnt, cin, cout, hw, stride in [
            (3, 64, 64, 56, 1),
            (1, 128, 128, 56, 2), (3, 128, 128, 28, 1),
            (1, 256, 256, 28, 2), (5, 256, 256, 14, 1),
            (1, 512, 512, 14, 2), (2, 512, 512, 7, 1)]:
        torch.manual_seed(0)
        ho = (hw + 2 - 3) // stride + 1
        gy2d = torch.randn(n * ho * ho, cout, device="cuda").bfloat16()
        w2d = (torch.randn(cout, 9 * cin, device="cuda")
               * (9 * cin) ** -0.5).bfloat16()
        off = lambda: _C.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d, False,
                                       False, False)
        on = lambda: _C.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d, False,
                                      True, True)
        same = torch.equal(off(), on())
        # interleave the two variants; keep the faster of two rounds each
        t = {"off": 1e9, "on": 1e9}
        for _ in range(2):
            t["off"] = min(t["off"], time_fn(off))
            t["on"] = min(t["on"], time_fn(on))
        flops = 2.0 * n * ho * ho * cout * 9 * cin
        print(f"dgrad x{cnt} c={cin}->{cout} hw={hw} s={stride}: "
              f"off {t['off']*1e6:7.1f} us ({flops/t['off']/1e12:6.1f} TF) | "
              f"on {t['on']*1e6:7.1f} us ({flops/t['on']/1e12:6.1f} TF) "
              f"{'equal' if same else 'DIFFERENT'}", flush=True)
        for k in tot:
            tot[k] += cnt * t[k]
    print(f"dgrad per step (weighted): off {tot['off']*1e6:.0f} us  "
          f"on {tot['on']*1e6:.0f} us")
    # layer-1 forward, 128- vs 64-wide n-tile
    cin = cout = 64
    hw = 56
    x2d = torch.randn(n * hw * hw, cin, device="cuda").bfloat16()
    w2d = (torch.randn(cout, 9 * cin, device="cuda")
           * (9 * cin) ** -0.5).bfloat16()
    f128 = lambda: _C.conv3x3_fwd_stats(x2d, n, hw, hw, 1, w2d, False, False)
    f64 = lambda: _C.conv3x3_fwd_stats(x2d, n, hw, hw, 1, w2d, False, True)
    same = all(torch.equal(a, b) for a, b in zip(f128(), f64()))
    t128 = min(time_fn(f128), time_fn(f128))
    t64 = min(time_fn(f64), time_fn(f64))
    print(f"fwd+stats x3 c=64->64 hw=56 s=1: NT128 {t128*1e6:7.1f} us | "
          f"NT64 {t64*1e6:7.1f} us {'equal' if same else 'DIFFERENT'}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--dgrad-split":
        dgrad_split(int(sys.argv[2]) if len(sys.argv) > 2 else 512)
        sys.exit(0)
    run(512, 256, 256, 14)   # layer3 3x3 (K=2304)
    run(512, 512, 512, 7)    # layer4 3x3 (K=4608)
    run(512, 128, 128, 28)   # layer2 3x3 (K=1152)
    run(128, 256, 256, 14)
