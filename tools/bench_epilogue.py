"""A/B of the three C-store epilogues (AMDTRAIN_EPILOGUE 0 / 1 / 2) per
shape, in ONE process: every shape is timed in all three modes, the modes
alternated over several rounds and the fastest round kept, so clock drift
and box-to-box differences cancel.  Covers the 1x1-conv GEMM shapes of
tools/bench_conv1x1.py (forward with statistics, and the plain call the
dgrad makes), every ResNet-50 conv3x3 site (forward with statistics, dgrad)
and the stem forward.

    python tools/bench_epilogue.py [batch] [--json OUT]

1x1 rows also print min-traffic TB/s (A + B read once, C written once)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402

MODES = (0, 1, 2)
ROUNDS = 3


def time_fn(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def ab(call):
    """call(epi) -> thunk; returns {mode: best seconds}"""
    fns = {m: call(m) for m in MODES}
    best = {m: 1e9 for m in MODES}
    for _ in range(ROUNDS):
        for m in MODES:
            best[m] = min(best[m], time_fn(fns[m]))
    return best


def fmt(t, extra=""):
    cells = " | ".join(f"{t[m] * 1e6:7.1f}" for m in MODES)
    return f"{cells} | {t[0] / t[1]:5.3f} | {t[0] / t[2]:5.3f} |{extra}"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 512
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv \
        else None
    rows = []
    torch.manual_seed(0)
    hdr = "us mode0 | mode1 | mode2 | 0/1 | 0/2 |"
    print(f"== 1x1 GEMM shapes at b{B}: {hdr} TB/s min-traffic 0 / 1 / 2")
    for tag, M, N, K in [
            ("L1 c1",  B * 56 * 56, 64, 64), ("L1 c1'", B * 56 * 56, 64, 256),
            ("L1 c3",  B * 56 * 56, 256, 64),
            ("L2 c1",  B * 28 * 28, 128, 512), ("L2 c3", B * 28 * 28, 512, 128),
            ("L3 c1",  B * 14 * 14, 256, 1024),
            ("L3 c3",  B * 14 * 14, 1024, 256),
            ("L4 c1",  B * 7 * 7, 512, 2048), ("L4 c3", B * 7 * 7, 2048, 512)]:
        A = torch.randn(M, K, device="cuda").bfloat16()
        Bm = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
        by = 2.0 * (M * K + N * K + M * N)
        for kind, call in [
                ("stats", lambda e: lambda: _C.gemm_bt_stats(A, Bm, e)),
                ("plain", lambda e: lambda: _C.gemm_bt(A, Bm, False, None,
                                                       None, e))]:
            t = ab(call)
            tb = " / ".join(f"{by / t[m] / 1e12:4.2f}" for m in MODES)
            print(f"| {tag:6s} {kind} M={M} N={N} K={K} | {fmt(t, ' ' + tb)}",
                  flush=True)
            rows.append({"family": "gemm", "site": tag, "kind": kind, "M": M,
                         "N": N, "K": K, "us": [t[m] * 1e6 for m in MODES]})
        del A, Bm

    print(f"== conv3x3 sites at b{B} (calls per step): {hdr}")
    tot = {k: {m: 0.0 for m in MODES} for k in ("fwd", "dgrad")}
    for cnt, c, hw, stride in [(3, 64, 56, 1), (1, 128, 56, 2),
                               (3, 128, 28, 1), (1, 256, 28, 2),
                               (5, 256, 14, 1), (1, 512, 14, 2),
                               (2, 512, 7, 1)]:
        ho = (hw + 2 - 3) // stride + 1
        x2d = torch.randn(B * hw * hw, c, device="cuda").bfloat16()
        gy2d = torch.randn(B * ho * ho, c, device="cuda").bfloat16()
        w2d = (torch.randn(c, 9 * c, device="cuda") * (9 * c) ** -0.5) \
            .bfloat16()
        for kind, call in [
                ("fwd", lambda e: lambda: _C.conv3x3_fwd_stats(
                    x2d, B, hw, hw, stride, w2d, False, True, e)),
                ("dgrad", lambda e: lambda: _C.conv3x3_dgrad(
                    gy2d, B, hw, hw, stride, w2d, False, True, True, e))]:
            t = ab(call)
            print(f"| {kind:5s} x{cnt} c={c} hw={hw} s={stride} | {fmt(t)}",
                  flush=True)
            for m in MODES:
                tot[kind][m] += cnt * t[m]
            rows.append({"family": "conv3x3", "kind": kind, "calls": cnt,
                         "c": c, "hw": hw, "stride": stride,
                         "us": [t[m] * 1e6 for m in MODES]})
        del x2d, gy2d, w2d
    for kind in tot:
        print(f"| {kind} per step (weighted) | {fmt(tot[kind])}")

    print(f"== stem forward (49 taps, 3->8 channels, 64-wide tile) at b{B}: "
          f"{hdr}")
    H = 224
    x8 = torch.zeros(B * H * H, 8, device="cuda", dtype=torch.bfloat16)
    x8[:, :3] = torch.randn(B * H * H, 3, device="cuda").bfloat16()
    w8 = torch.zeros(64, 416, device="cuda", dtype=torch.bfloat16)
    w8[:, :392] = (torch.randn(64, 392, device="cuda") * 147 ** -0.5) \
        .bfloat16()
    t = ab(lambda e: lambda: _C.conv_generic_fwd(
        x8, B, H, H, 7, 7, 2, 3, w8, 0, -1, 0, 0, True, e))
    print(f"| stem fwd | {fmt(t)}", flush=True)
    rows.append({"family": "stem", "kind": "fwd",
                 "us": [t[m] * 1e6 for m in MODES]})
    if out:
        with open(out, "w") as fh:
            json.dump({"batch": B, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
