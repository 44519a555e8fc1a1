"""Micro-benchmark: the tn2_wgrad tr-read TN core (wgrad.hip) on the
ResNet-50 b512 weight-gradient shapes, refchecked against fp32 matmul /
conv2d_weight.

``--stem`` instead times the 7x7 stem at batch BENCH_B: the 49-tap
channel-padded forward and wgrad against the width space-to-depth form,
whose wgrad runs on the (1,4,32) and, with AMDTRAIN_TN2_STEM22, the
(2,2,64) wave grid.

``--addr`` times every gathered-X wgrad of the step (3x3, strided 1x1,
both stem forms) with the direct address code (AMDTRAIN_TN2_ADDR=0) and
the incremental walk, alternated in one process; ``--configs`` times the
tile choices (AMDTRAIN_TN2_14, _STEM22; run it again under
AMDTRAIN_TN2_W8=0/1 and AMDTRAIN_TN2_PIPE3=1, which are read once)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from amdtrain import _C  # noqa: E402

B = int(os.environ.get("BENCH_B", "512"))


def time_fn(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def run_1x1(tag, M, N, K):
    torch.manual_seed(0)
    dY = torch.randn(M, N, device="cuda").bfloat16()
    X = torch.randn(M, K, device="cuda").bfloat16()
    ref = dY.float().t() @ X.float()
    err = (_C.tn2_wgrad(dY, X) - ref).abs().max().item()
    # both sides sum exact bf16 products in fp32: only the order differs
    ok = err < 1e-3 * ref.abs().max().item()
    t = time_fn(lambda: _C.tn2_wgrad(dY, X))
    tf = 2.0 * M * N * K
    print(f"1x1 {tag:22s} M={M:8d} N={N:4d} K={K:4d}  "
          f"{t*1e3:7.3f} ms ({tf/t/1e12:6.1f} TF)  "
          f"{'OK' if ok else 'REFCHECK FAIL err=%.3f' % err}")
    return t


def run_3x3(tag, n, c_in, c_out, hw, s):
    torch.manual_seed(0)
    ho = (hw + 2 - 3) // s + 1
    M = n * ho * ho
    x2d = torch.randn(n * hw * hw, c_in, device="cuda").bfloat16()
    gy2d = torch.randn(M, c_out, device="cuda").bfloat16()
    # refcheck on the first 4 images (the fp32 reference is slow at batch B)
    nr = min(n, 4)
    xr = x2d[:nr * hw * hw].float().view(nr, hw, hw, c_in).permute(0, 3, 1, 2)
    gr = gy2d[:nr * ho * ho].float().view(nr, ho, ho, c_out) \
        .permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xr, (c_out, c_in, 3, 3), gr, stride=s,
                                      padding=1)
    got = _C.tn2_wgrad(gy2d[:nr * ho * ho], x2d[:nr * hw * hw], 9, nr, hw,
                       hw, s, 2)
    err = (got.view(c_out, 3, 3, c_in).permute(0, 3, 1, 2) - ref) \
        .abs().max().item()
    ok = err < 0.5
    t = time_fn(lambda: _C.tn2_wgrad(gy2d, x2d, 9, n, hw, hw, s, 2))
    tf = 2.0 * M * c_out * 9 * c_in
    print(f"3x3 {tag:22s} M={M:8d} N={c_out:4d} K9={9*c_in:4d}  "
          f"{t*1e3:7.3f} ms ({tf/t/1e12:6.1f} TF)  "
          f"{'OK' if ok else 'REFCHECK FAIL err=%.3f' % err}")
    return t


def main():
    print(f"== ResNet-50 wgrad shapes at batch {B} ==")
    tot = 0.0
    # conv3x3 sites (count x shape per fwd pass)
    for cnt, (cin, cout, hw, s) in [
            (3, (64, 64, 56, 1)),
            (1, (128, 128, 56, 2)), (3, (128, 128, 28, 1)),
            (1, (256, 256, 28, 2)), (5, (256, 256, 14, 1)),
            (1, (512, 512, 14, 2)), (2, (512, 512, 7, 1))]:
        tot += cnt * run_3x3(f"{cin}->{cout} {hw}x{hw}/{s}", B, cin, cout,
                             hw, s)
    # 1x1 sites
    for cnt, (M, N, K) in [
            (1, (B * 56 * 56, 64, 64)), (2, (B * 56 * 56, 64, 256)),
            (3, (B * 56 * 56, 256, 64)),
            (1, (B * 56 * 56, 128, 256)), (3, (B * 28 * 28, 128, 512)),
            (4, (B * 28 * 28, 512, 128)),
            (1, (B * 28 * 28, 256, 512)), (5, (B * 14 * 14, 256, 1024)),
            (6, (B * 14 * 14, 1024, 256)),
            (1, (B * 14 * 14, 512, 1024)), (2, (B * 7 * 7, 512, 2048)),
            (3, (B * 7 * 7, 2048, 512))]:
        tot += cnt * run_1x1(f"{N}x{K}", M, N, K)
    print(f"\nTOTAL wgrad/step (weighted): {tot*1e3:.2f} ms")


def run_stem():
    import torch.nn.functional as F
    from amdtrain.ops.conv import stem_s2d_input, stem_s2d_weight
    torch.manual_seed(0)
    H = 224
    Ho = (H + 6 - 7) // 2 + 1
    M = B * Ho * Ho
    x = torch.randn(B, H, H, 3, device="cuda").bfloat16()
    w = (torch.randn(64, 3, 7, 7, device="cuda") * 147 ** -0.5).bfloat16()
    gy = torch.randn(M, 64, device="cuda").bfloat16()
    x8 = F.pad(x, (0, 5)).view(B * H * H, 8)
    w8 = F.pad(F.pad(w.permute(0, 2, 3, 1), (0, 5)).reshape(64, 392),
               (0, 24))
    xs = stem_s2d_input(x).view(B * H * (H // 2), 8)
    ws = stem_s2d_weight(w).reshape(64, 224)
    f_old = lambda: _C.conv_generic_fwd(x8, B, H, H, 7, 7, 2, 3, w8)
    f_new = lambda: _C.conv_generic_fwd_stats(xs, B, H, H // 2, 7, 4, 2, 3, ws,
                                              1, 2, Ho, Ho, True)
    g_old = lambda: _C.tn2_wgrad(gy, x8, 49, B, H, H, 2, 2, 7, 7, 3)
    g_new = lambda: _C.tn2_wgrad(gy, xs, 28, B, H, H // 2, 2, 2, 7, 4, 3,
                                 1, 2, Ho, Ho)
    f_old64 = lambda: _C.conv_generic_fwd(x8, B, H, H, 7, 7, 2, 3, w8,
                                          0, -1, 0, 0, True)
    print("stem fwd 49-tap NT64 vs NT128:",
          "equal" if torch.equal(f_old64(), f_old()) else "DIFFERENT")
    err = (f_new()[0].float() - f_old().float()).abs().max().item()
    print(f"stem fwd s2d vs 49-tap: max diff {err:.4f}")
    flops = 2.0 * M * 64 * 147
    for tag, fn in [("fwd 49-tap K=416 NT128", f_old),
                    ("fwd 49-tap K=416 NT64", f_old64),
                    ("fwd s2d K=224 NT64 +stats", f_new),
                    ("wgrad 49-tap (1,4,32) nbk=2", g_old),
                    ("wgrad s2d (1,4,32) nbk=1", g_new)]:
        t = min(time_fn(fn), time_fn(fn))
        print(f"{tag:30s} {t*1e6:8.1f} us  ({flops/t/1e12:6.1f} useful TF)",
              flush=True)
    os.environ["AMDTRAIN_TN2_STEM22"] = "1"
    t = min(time_fn(g_new), time_fn(g_new))
    del os.environ["AMDTRAIN_TN2_STEM22"]
    print(f"{'wgrad s2d (2,2,64) nbk=2':30s} {t*1e6:8.1f} us  "
          f"({flops/t/1e12:6.1f} useful TF)")


def ab_env(fn, variants, rounds=3, iters=30):
    """fn timed under each {env} of variants, alternated over rounds in
    this process (the tn2 switches named here are read per call); fastest
    round per variant, plus whether every variant returns the same bits"""
    best = {k: float("inf") for k in variants}
    outs = {}
    for _ in range(rounds):
        for k, env in variants.items():
            os.environ.update(env)
            outs[k] = fn()
            best[k] = min(best[k], time_fn(fn, iters))
            for name in env:
                del os.environ[name]
    ref = next(iter(outs.values()))
    same = all(torch.equal(ref, o) for o in outs.values())
    return best, same


def gather_sites():
    """(label, calls per step, flops, call) of every gathered-X wgrad of a
    ResNet-50 step at batch B: the 3x3 convs, both stem forms and the
    strided 1x1 downsample convs"""
    from amdtrain.ops.conv import stem_s2d_input
    sites = []
    for cnt, (cin, cout, hw, s) in [
            (3, (64, 64, 56, 1)),
            (1, (128, 128, 56, 2)), (3, (128, 128, 28, 1)),
            (1, (256, 256, 28, 2)), (5, (256, 256, 14, 1)),
            (1, (512, 512, 14, 2)), (2, (512, 512, 7, 1))]:
        ho = (hw + 2 - 3) // s + 1
        M = B * ho * ho
        x2d = torch.randn(B * hw * hw, cin, device="cuda").bfloat16()
        gy2d = torch.randn(M, cout, device="cuda").bfloat16()
        sites.append((
            f"3x3 {cin}->{cout} {hw}x{hw}/{s}", cnt, 2.0 * M * cout * 9 * cin,
            lambda gy2d=gy2d, x2d=x2d, hw=hw, s=s:
                _C.tn2_wgrad(gy2d, x2d, 9, B, hw, hw, s, 2)))
    for cin, cout, hw in [(256, 512, 56), (512, 1024, 28), (1024, 2048, 14)]:
        M = B * (hw // 2) ** 2
        x2d = torch.randn(B * hw * hw, cin, device="cuda").bfloat16()
        gy2d = torch.randn(M, cout, device="cuda").bfloat16()
        sites.append((
            f"1x1/2 {cin}->{cout} {hw}x{hw}", 1, 2.0 * M * cout * cin,
            lambda gy2d=gy2d, x2d=x2d, hw=hw:
                _C.tn2_wgrad(gy2d, x2d, 1, B, hw, hw, 2, 1)))
    H = 224
    Ho = H // 2
    gy = torch.randn(B * Ho * Ho, 64, device="cuda").bfloat16()
    x = torch.randn(B, H, H, 3, device="cuda").bfloat16()
    x8 = torch.nn.functional.pad(x, (0, 5)).view(B * H * H, 8)
    xs = stem_s2d_input(x).view(B * H * (H // 2), 8)
    flops = 2.0 * B * Ho * Ho * 64 * 147
    sites.append(("stem 49-tap", 1, flops,
                  lambda: _C.tn2_wgrad(gy, x8, 49, B, H, H, 2, 2, 7, 7, 3)))
    sites.append(("stem s2d 28-tap (not default)", 0, flops,
                  lambda: _C.tn2_wgrad(gy, xs, 28, B, H, H // 2, 2, 2, 7, 4,
                                       3, 1, 2, Ho, Ho)))
    return sites


def run_addr():
    """AMDTRAIN_TN2_ADDR=0 (every address derived from m) against the
    incremental walk, and the walk with AMDTRAIN_TN2_NSKIP=0"""
    torch.manual_seed(0)
    variants = {"direct": {"AMDTRAIN_TN2_ADDR": "0"},
                "walk": {"AMDTRAIN_TN2_ADDR": "1"},
                "walk, no N skip": {"AMDTRAIN_TN2_NSKIP": "0"}}
    print(f"== gathered-X wgrads at batch {B}: us (useful TF) ==")
    print("| site (calls/step) | " + " | ".join(variants) + " | same bits |")
    print("|---|" + "---|" * (len(variants) + 1))
    tot = {k: 0.0 for k in variants}
    for label, cnt, flops, fn in gather_sites():
        best, same = ab_env(fn, variants)
        for k in variants:
            tot[k] += cnt * best[k]
        cells = [f"{best[k]*1e6:.1f} ({flops/best[k]/1e12:.0f})"
                 for k in variants]
        print(f"| {label} ({cnt}) | " + " | ".join(cells) +
              f" | {'yes' if same else 'NO'} |", flush=True)
    print("| weighted per step | " +
          " | ".join(f"{tot[k]*1e6:.0f}" for k in variants) + " | |")


def run_configs():
    """The tile decisions taken while the m-loop was address-bound, timed
    again on the walk.  AMDTRAIN_TN2_W8 and AMDTRAIN_TN2_PIPE3 are read
    once per process: set them outside and compare the 'default' column
    across runs."""
    torch.manual_seed(0)
    variants = {"default": {}, "TN2_14": {"AMDTRAIN_TN2_14": "1"},
                "STEM22": {"AMDTRAIN_TN2_STEM22": "1"}}
    held = {k: os.environ[k] for k in ("AMDTRAIN_TN2_W8", "AMDTRAIN_TN2_PIPE3")
            if k in os.environ}
    print(f"== tn2 configurations at batch {B}, process-wide {held}: us ==")
    print("| site | " + " | ".join(variants) + " |")
    print("|---|" + "---|" * len(variants))
    for label, cnt, flops, fn in gather_sites():
        best, _ = ab_env(fn, variants)
        print(f"| {label} | " +
              " | ".join(f"{best[k]*1e6:.1f}" for k in variants) + " |",
              flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--stem":
        run_stem()
    elif len(sys.argv) > 1 and sys.argv[1] == "--addr":
        run_addr()
    elif len(sys.argv) > 1 and sys.argv[1] == "--configs":
        run_configs()
    else:
        main()
