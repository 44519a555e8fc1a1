"""Pointwise MFMA GEMM on the 8 grid (pwgemm8.hip) against fp64 arithmetic on
the bf16 input values.  With ref = A B^T and S = |A| |B|^T the bounds are the
derived ones of test_gpu_pwconv.py, not measured:
  C:     |C - ref| <= 2^-8 |ref| + (K+1) 2^-23 S;  layer dX: (K, N) swapped
  stats: |sum - sum_m ref| <= (K+M) 2^-23 sum_m S,
         |sumsq - sum_m ref^2| <= (2K+M+2) 2^-23 sum_m S^2
  dW:    |dW - ref| <= (M+1) 2^-23 |dY|^T |X|
Inputs are random and asymmetric, so a transposed C map cannot pass."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U23 = 2.0 ** -23
# every K tail and N tail (0, 8, 16, 24 mod 32), one and many k-steps, one
# and many n-tiles, both instances (n-tile 64 for N <= 64, else 128)
PAIRS = [(40, 240), (240, 40), (88, 528), (528, 136), (816, 224), (288, 72),
         (480, 80), (264, 8), (8, 264)]
CONV_ENV = ("AMDTRAIN_CONV1X1", "AMDTRAIN_CONV3X3", "AMDTRAIN_CONVSTEM",
            "AMDTRAIN_DWCONV")


def _check(name, out, ref, bound):
    out = out.detach().double().cpu()
    err = (out - ref).abs()
    print(f"{name}: max err {err.max().item():.3e}, max err/bound "
          f"{(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert out.shape == ref.shape and torch.isfinite(out).all(), name
    assert (err <= bound).all(), \
        f"{name}: worst excess {(err - bound).max().item():.3e}"


def _c_bound(ref, s, k):
    return 2.0 ** -8 * ref.abs() + (k + 1) * U23 * s


@functools.lru_cache(maxsize=None)
def _case(m, k, n):
    """Seeded operands and their fp64 reference, shared read-only."""
    g = torch.Generator().manual_seed(1000003 * m + 1009 * k + n)
    a = torch.randn(m, k, generator=g).bfloat16()
    b = (torch.randn(n, k, generator=g) * k ** -0.5).bfloat16()
    return a, b, a.double() @ b.double().t(), \
        a.double().abs() @ b.double().abs().t()


def _run_kernel(m, k, n, want_stats, n_tile=0):
    """Runs and checks.  A is the first M rows of a buffer whose other rows
    are NaN: a row or k-pack that is over-read, not zeroed, shows in C."""
    from amdtrain import _C
    a, b, ref, s = _case(m, k, n)
    big = torch.full((m + 300, k), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    big[:m] = a.to(DEV)
    c, stats = _C.pw8_gemm(big[:m], b.to(DEV), want_stats, n_tile)
    torch.cuda.synchronize()
    assert c.dtype == torch.bfloat16
    _check("C", c, ref, _c_bound(ref, s, k))
    if not want_stats:
        assert stats.numel() == 0
        return c, stats
    assert stats.dtype == torch.float32
    assert tuple(stats.shape) == ((m + 127) // 128, 2 * n)
    tot = stats.double().cpu().sum(0)
    _check("sum", tot[:n], ref.sum(0), (k + m) * U23 * s.sum(0))
    _check("sumsq", tot[n:], (ref * ref).sum(0),
           (2 * k + m + 2) * U23 * (s * s).sum(0))
    return c, stats


# edge M: 129 is one row above the 128-row block tile, 257 two tiles and a row
@pytest.mark.parametrize("m,k,n,want_stats", [
    (777, k, n, st) for k, n in PAIRS for st in (False, True)] + [
    (m, k, n, True) for m in (1, 15, 129, 257)
    for k, n in ((88, 528), (528, 88))])
def test_kernel_vs_fp64(m, k, n, want_stats):
    _run_kernel(m, k, n, want_stats)


@pytest.mark.parametrize("k,n", [(528, 136), (88, 528)])
def test_bitwise_repeat(k, n):
    """No atomics, a grid that depends on the shape and constants only; the
    other instance (several 64-wide n-tiles) keeps every k and row order."""
    c1, s1 = _run_kernel(777, k, n, True)
    for n_tile in (0, 64):
        c2, s2 = _run_kernel(777, k, n, True, n_tile)
        assert torch.equal(c1, c2) and torch.equal(s1, s2)


def test_host_contract():
    from amdtrain import _C

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, dtype=dtype, device=DEV)

    for a, b in [(z(64, 44), z(16, 44)),                      # K % 8
                 (z(64, 48), z(20, 48)),                      # N % 8
                 (z(64, 48, dtype=torch.float32),
                  z(88, 48, dtype=torch.float32)),            # dtype
                 (z(64, 48), z(88, 56))]:                     # K mismatch
        with pytest.raises(RuntimeError):
            _C.pw8_gemm(a, b, False)
    for want_stats in (True, False):                          # no launch
        c, stats = _C.pw8_gemm(z(0, 48), z(88, 48), want_stats)
        assert tuple(c.shape) == (0, 88) and c.dtype == torch.bfloat16
        assert stats.numel() == 0
    torch.cuda.synchronize()


def _spy(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)
    monkeypatch.setattr(owner, name,
                        lambda *a, **kw: calls.append(name) or real(*a, **kw))
    return calls


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def _layer_case(cin, cout):
    g = torch.Generator().manual_seed(7919 * cin + cout)
    x = torch.randn(2, cin, 5, 7, generator=g).bfloat16()
    w = (torch.randn(cout, cin, 1, 1, generator=g) * cin ** -0.5).bfloat16()
    go = torch.randn(2, cout, 5, 7, generator=g).bfloat16()
    out = dict(x=x, w=w, go=go)
    # the conv itself, then |dY|^T |X| and |dY| |W| as the gradients of the
    # all-absolute conv
    for tag, f in (("", torch.Tensor.double),
                   ("s_", lambda t: t.double().abs())):
        xd, wd = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y = F.conv2d(xd, wd)
        y.backward(f(go))
        out.update({tag + "y": y.detach(), tag + "dx": xd.grad,
                    tag + "dw": wd.grad})
    return out


def _run_layer(k, cin, cout):
    """fp32 master weight holding bf16 values, under autocast, as in
    training: the weight gradient arrives in fp32."""
    from amdtrain.ops.conv import AmdConv2d
    conv = AmdConv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(k["w"].float())
    conv = conv.to(DEV)
    x = _nhwc(k["x"]).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv(x)
    y.backward(_nhwc(k["go"]))
    torch.cuda.synchronize()
    return y, x.grad, conv.weight.grad


def _default_env(monkeypatch):
    for name in CONV_ENV + ("AMDTRAIN_PWWIDE", "AMDTRAIN_PWCONV"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("AMDTRAIN_FUSE_BNSTATS", "1")


# (480, 80) and (288, 48) raised in backward before the kernel
@pytest.mark.parametrize("cin,cout", [(480, 80), (288, 48), (88, 528),
                                      (240, 40)])
def test_layer(monkeypatch, cin, cout):
    from amdtrain import _C
    _default_env(monkeypatch)
    wide = _spy(monkeypatch, _C, "pw8_gemm")
    others = [_spy(monkeypatch, _C, name)
              for name in ("gemm_bt", "gemm_bt_stats", "pw_gemm")]
    k = _layer_case(cin, cout)
    y, dx, dw = _run_layer(k, cin, cout)
    assert len(wide) == 2 and others == [[], [], []]
    assert (y.dtype, dx.dtype, dw.dtype) \
        == (torch.bfloat16, torch.bfloat16, torch.float32)
    assert y._amdtrain_bn_stats.size(1) == 2 * cout
    _check("y", y, k["y"], _c_bound(k["y"], k["s_y"], cin))
    _check("dx", dx, k["dx"], _c_bound(k["dx"], k["s_dx"], cout))
    _check("dw", dw, k["dw"], (2 * 5 * 7 + 1) * U23 * k["s_dw"])


def test_bn_takes_the_partials(monkeypatch):
    from amdtrain import _C
    from amdtrain.models.resnet import FusedBatchNorm2d
    from amdtrain.ops import fused
    from amdtrain.ops.conv import AmdConv2d
    _default_env(monkeypatch)
    from_parts = _spy(monkeypatch, _C, "batch_norm_fwd_train_from_parts")
    own_stats = _spy(monkeypatch, _C, "batch_norm_train_stats")
    cin, cout = 88, 528
    k = _layer_case(cin, cout)
    conv = AmdConv2d(cin, cout, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(k["w"].float())
    conv = conv.to(DEV).to(torch.bfloat16)
    bn = FusedBatchNorm2d(cout).to(DEV).train()
    with torch.no_grad():
        y = fused.batch_norm(conv(_nhwc(k["x"])), bn, relu6=True)
    torch.cuda.synchronize()
    assert len(from_parts) == 1 and own_stats == []
    assert torch.isfinite(y).all() and torch.isfinite(bn.running_var).all()


def test_switch_off(monkeypatch):
    from amdtrain import _C
    _default_env(monkeypatch)
    monkeypatch.setenv("AMDTRAIN_PWWIDE", "0")
    wide = _spy(monkeypatch, _C, "pw8_gemm")
    y, dx, _ = _run_layer(_layer_case(40, 240), 40, 240)
    assert wide == [] and torch.isfinite(y).all() and torch.isfinite(dx).all()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _step_140():
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    torch.manual_seed(0)
    m = build_model("mobilenet_v2_140").to(DEV) \
        .to(memory_format=torch.channels_last).train()
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    x_cpu, t_cpu = torch.randn(4, 3, 64, 64), torch.randint(0, 1000, (4,))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = CrossEntropyLoss()(m(_nhwc(x_cpu)), t_cpu.to(DEV))
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return m, before, loss, x_cpu, t_cpu


def test_model_step(monkeypatch):
    import amdtrain.ops.conv as conv_mod
    from amdtrain.models import build_model
    _default_env(monkeypatch)
    lib = _spy(monkeypatch, F, "conv2d")
    wide = _spy(monkeypatch, conv_mod, "conv1x1_wide")
    m, before, loss, x_cpu, t_cpu = _step_140()
    assert torch.isfinite(loss).item()
    assert lib == [] and len(wide) == 21
    same = [k for k, v in m.named_parameters() if torch.equal(v, before[k])]
    assert not same, same
    again = _step_140()[0].state_dict()
    diff = [k for k, v in m.state_dict().items()
            if not torch.equal(v, again[k])]
    assert not diff, diff
    # the comparison of test_gpu_dwconv.py::test_model_step: an fp32 CPU copy
    # of the weights as they stand, dropout off (its mask differs by device
    # and call), everything else in train mode
    m.classifier[0].p = 0.0
    ref = build_model("mobilenet_v2_140")
    ref.load_state_dict({k: v.detach().cpu() for k, v in
                         m.state_dict().items()})
    ref.train()
    ref.classifier[0].p = 0.0
    out_ref = ref(x_cpu).detach()
    loss_ref = F.cross_entropy(out_ref, t_cpu, reduction="none")

    def gpu_pass():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(_nhwc(x_cpu)).float().cpu()
        return (_rel(out, out_ref),
                _rel(F.cross_entropy(out, t_cpu, reduction="none"), loss_ref))

    e_custom = gpu_pass()
    for name in CONV_ENV:
        monkeypatch.setenv(name, "miopen")
    e_lib = gpu_pass()
    print(f"logits: e_custom {e_custom[0]:.4e} e_lib {e_lib[0]:.4e}")
    print(f"loss:   e_custom {e_custom[1]:.4e} e_lib {e_lib[1]:.4e}")
    assert e_custom[0] <= 2 * e_lib[0] and e_custom[1] <= 2 * e_lib[1]
