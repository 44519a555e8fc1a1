"""Grouped 3x3 convs of resnext50_32x4d at batch 256: per-call time of the
forward with statistics, of the input gradient and of the weight gradient,
per-group kernels (gconv.hip, gconv_wgrad.hip) against the banded dense path,
each with what a training step pays around it (one pack launch / the eager
dense expansion; for the banded weight gradient the eager extraction of the
group diagonal).  The two are alternated in one process and compared.
``AMDTRAIN_BENCH_NSPLIT`` forces the weight-gradient kernel's split.

Without arguments every shape runs in a child process of its own under a
time limit, and the run stops at the first child that fails;
``--shape I`` runs one shape."""
import os
import subprocess
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCH = 256
GROUPS = 32
# (sites per step, C, input H = W, stride)
SHAPES = [(3, 128, 56, 1), (1, 256, 56, 2), (3, 256, 28, 1), (1, 512, 28, 2),
          (5, 512, 14, 1), (1, 1024, 14, 2), (2, 1024, 7, 1)]


def time_fn(fn, iters=20):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def run(idx):
    import torch
    from amdtrain import _C
    from amdtrain.ops.conv import _grouped_dw
    nsplit = int(os.environ.get("AMDTRAIN_BENCH_NSPLIT", "0"))
    cnt, c, hw, stride = SHAPES[idx]
    n, s = BATCH, c // GROUPS
    ho = (hw + 2 - 3) // stride + 1
    torch.manual_seed(0)
    x2d = torch.randn(n * hw * hw, c, device="cuda").bfloat16()
    gy2d = torch.randn(n * ho * ho, c, device="cuda").bfloat16()
    w = (torch.randn(c, s, 3, 3, device="cuda") * (9 * s) ** -0.5) \
        .bfloat16().contiguous(memory_format=torch.channels_last)

    def dense():
        wg = w.permute(0, 2, 3, 1).reshape(GROUPS, s, 3, 3, s)
        d = torch.zeros(GROUPS, s, 3, 3, GROUPS, s, dtype=w.dtype,
                        device=w.device)
        gi = torch.arange(GROUPS, device=w.device)
        d[gi, :, :, :, gi, :] = wg
        return d.reshape(c, 9 * c)

    w2d = dense()
    fns = {
        "fwd": {
            "banded": lambda: _C.conv3x3_fwd_stats(x2d, n, hw, hw, stride,
                                                   dense(), True),
            "group": lambda: _C.gconv3x3_fwd(
                x2d, n, hw, hw, stride, _C.gconv3x3_pack(w, GROUPS, False),
                GROUPS, True)},
        "dgrad": {
            "banded": lambda: _C.conv3x3_dgrad(gy2d, n, hw, hw, stride, w2d,
                                               True),
            "group": lambda: _C.gconv3x3_dgrad(
                gy2d, n, hw, hw, stride, _C.gconv3x3_pack(w, GROUPS, True),
                GROUPS)},
        "wgrad": {
            "banded": lambda: _grouped_dw(_C, gy2d, x2d, n, hw, hw, stride, c,
                                          GROUPS, True),
            "group": lambda: _C.gconv3x3_wgrad(gy2d, x2d, n, hw, hw, stride,
                                               GROUPS, nsplit)}}
    # bytes the op must move (read + write once) and the flops it contains
    byts = 2.0 * c * n * (hw * hw + ho * ho)
    flops = 2.0 * n * ho * ho * c * 9 * s
    for op, pair in fns.items():
        a, b = pair["banded"](), pair["group"]()
        a, b = (a[0], b[0]) if op == "fwd" else (a, b)
        diff = (a.float() - b.float()).abs().max().item()
        # interleave the two paths; keep the faster of two rounds each
        t = {k: 1e9 for k in pair}
        for _ in range(2):
            for k, fn in pair.items():
                t[k] = min(t[k], time_fn(fn))
        print(f"{op:5s} x{cnt} C={c} S={s} hw={hw} s={stride}: "
              f"banded {t['banded']*1e6:7.1f} us | group "
              f"{t['group']*1e6:7.1f} us ({byts/t['group']/1e12:5.2f} TB/s, "
              f"{flops/t['group']/1e12:5.1f} useful TF) "
              f"max|diff| {diff:.4f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--shape":
        run(int(sys.argv[2]))
        sys.exit(0)
    for i in range(len(SHAPES)):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__),
                             "--shape", str(i)], timeout=120).returncode
        if rc != 0:
            sys.exit(f"shape {i} failed with exit code {rc}")
