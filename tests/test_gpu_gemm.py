"""GPU tests for the MFMA GEMM kernels and the 1x1-conv path built on them,
verified against torch.matmul / F.conv2d fp32 references with random
asymmetric inputs (transpose-detecting, per the CDNA4 guide's G9 rule)."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available()
    from amdtrain import _C
    return _C


@pytest.mark.parametrize("M,N,K", [
    (256, 128, 64),       # exact tiles
    (100, 64, 64),        # ragged M, small N
    (1000, 256, 512),     # ragged M
    (3136, 2048, 512),    # a real ResNet-50 shape (B=1 layer4 expand)
])
def test_gemm_bt_matches_matmul(M, N, K):
    e = _ext()
    torch.manual_seed(0)
    A = torch.randn(M, K, device=DEV).bfloat16()
    B = torch.randn(N, K, device=DEV).bfloat16()
    C = e.gemm_bt(A, B, True)  # f32 out
    ref = A.float() @ B.float().t()
    assert C.shape == (M, N)
    err = (C - ref).abs()
    tol = 0.02 * ref.abs().mean().item() + 0.05
    assert err.max().item() < max(tol * 10, 0.5), \
        f"max err {err.max().item()} mean {err.mean().item()}"
    assert torch.allclose(C, ref, atol=0.5, rtol=0.05)


def test_gemm_bt_bf16_out():
    e = _ext()
    torch.manual_seed(1)
    A = torch.randn(512, 128, device=DEV).bfloat16()
    B = torch.randn(128, 128, device=DEV).bfloat16()
    C = e.gemm_bt(A, B, False)
    assert C.dtype == torch.bfloat16
    ref = (A.float() @ B.float().t())
    assert torch.allclose(C.float(), ref, atol=0.5, rtol=0.05)


@pytest.mark.parametrize("M,N,K", [
    (512, 128, 128),
    (3000, 256, 64),
    (12544, 512, 128),    # wgrad shape: dW[512,128] over M=B*H*W
])
def test_tn2_plain_matches_matmul(M, N, K):
    """The plain-rows tn2_wgrad (the 1x1-conv weight gradient) vs matmul."""
    e = _ext()
    torch.manual_seed(2)
    dY = (torch.randn(M, N, device=DEV) / (M ** 0.25)).bfloat16()
    X = (torch.randn(M, K, device=DEV) / (M ** 0.25)).bfloat16()
    dW = e.tn2_wgrad(dY, X)
    ref = dY.float().t() @ X.float()
    assert dW.shape == (N, K)
    denom = ref.abs().mean().item() + 1e-3
    rel = (dW - ref).abs().max().item() / denom
    assert rel < 0.3, f"relative max err {rel}"
    assert torch.allclose(dW, ref, atol=denom * 0.2 + 0.5, rtol=0.05)


def test_transpose_2d():
    e = _ext()
    x = torch.randn(130, 70, device=DEV).bfloat16()
    y = e.transpose_2d(x)
    assert torch.equal(y, x.t().contiguous())


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout", [(64, 256), (512, 128), (1024, 2048)])
def test_conv1x1_mfma_vs_miopen(stride, cin, cout):
    from amdtrain.ops.conv import conv1x1_mfma
    _ext()
    torch.manual_seed(3)
    x = torch.randn(2, cin, 14, 14, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    w = torch.randn(cout, cin, 1, 1, device=DEV) * (cin ** -0.5)

    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = conv1x1_mfma(xg, wg, stride)
    g = torch.randn_like(y.float())
    y.float().backward(g)

    xr = x.clone().float().requires_grad_(True)
    wr = w.clone().float().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=stride)
    yr.backward(g)

    assert y.shape == yr.shape
    assert torch.allclose(y.float(), yr, atol=0.3, rtol=0.05), \
        (y.float() - yr).abs().max()
    assert torch.allclose(xg.grad.float(), xr.grad, atol=0.5, rtol=0.1), \
        (xg.grad.float() - xr.grad).abs().max()
    assert torch.allclose(wg.grad, wr.grad, atol=1.0, rtol=0.1), \
        (wg.grad - wr.grad).abs().max()


def test_resnet50_custom_conv1x1_step(monkeypatch):
    """Full flagship step with the MFMA 1x1 path enabled."""
    monkeypatch.setenv("AMDTRAIN_CONV1X1", "custom")
    from amdtrain.models import build_model
    from amdtrain.ops import CrossEntropyLoss, FusedSGD
    _ext()
    torch.manual_seed(4)
    m = build_model("resnet50").to(DEV).to(memory_format=torch.channels_last)
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9)
    x = torch.randn(4, 3, 224, 224, device=DEV) \
        .contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 1000, (4,), device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(x)
    loss = CrossEntropyLoss()(out, t)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()


@pytest.mark.parametrize("fn_name", ["gemm_bt_8p3"])
def test_gemm_8p_variants_match_matmul(fn_name):
    """The experimental 256x256-tile kernel (top of the square-GEMM ladder,
    976 TF @4096^3) stays correct."""
    e = _ext()
    torch.manual_seed(7)
    for M, N, K in [(512, 512, 128), (1000, 256, 256), (2048, 512, 192)]:
        A = torch.randn(M, K, device=DEV).bfloat16()
        B = torch.randn(N, K, device=DEV).bfloat16()
        C = e.gemm_bt_8p3(A, B).float()  # fn_name: the one variant left
        ref = A.float() @ B.float().t()
        assert torch.allclose(C, ref, atol=0.5, rtol=0.05), \
            (C - ref).abs().max()


def test_amd_linear_parity():
    """FC classifier (fwd bias epilogue + dgrad pad + tn2 wgrad) vs fp32
    F.linear — retires the last library GEMM on the hot path."""
    import torch.nn.functional as F
    from amdtrain.ops.linear import AmdLinear

    torch.manual_seed(0)
    lin = AmdLinear(2048, 1000).cuda()
    x = torch.randn(256, 2048, device="cuda")
    # fp32 reference
    xr = x.clone().requires_grad_(True)
    wr = lin.weight.detach().clone().requires_grad_(True)
    br = lin.bias.detach().clone().requires_grad_(True)
    yr = F.linear(xr, wr, br)
    gy = torch.randn_like(yr)
    yr.backward(gy)
    # custom path under autocast
    xc = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = lin(xc)
    assert y.dtype == torch.bfloat16
    y.backward(gy.bfloat16())
    assert torch.allclose(y.float(), yr, atol=2.0, rtol=0.05)
    assert torch.allclose(xc.grad.float(), xr.grad, atol=2.0, rtol=0.05)
    assert torch.allclose(lin.weight.grad, wr.grad, atol=2.0, rtol=0.05)
    assert torch.allclose(lin.bias.grad, br.grad, atol=1.0, rtol=0.05)


def test_gemm_bt_dual_n_tile():
    """Wide-N small-K dual-n-tile variant (A-panel reuse) vs matmul, plus
    its fused BN-stats epilogue vs direct column sums."""
    from amdtrain import _C
    torch.manual_seed(0)
    M, N, K = 40960 + 96, 256, 64  # ragged M; grid large enough to engage
    A = torch.randn(M, K, device="cuda").bfloat16()
    B = torch.randn(N, K, device="cuda").bfloat16()
    y = _C.gemm_bt(A, B, False)
    ref = (A.float() @ B.float().t())
    assert torch.allclose(y.float(), ref, atol=1.0, rtol=0.02), \
        (y.float() - ref).abs().max().item()
    y2, stats = _C.gemm_bt_stats(A, B)
    assert torch.equal(y2, y)
    s1 = stats[:, :N].sum(0)
    s2 = stats[:, N:].sum(0)
    yf = y.float()
    # stats accumulate the fp32 accumulators; yf is the bf16-ROUNDED output,
    # so the column sums random-walk apart by ~0.02*sqrt(M) (~4 at M=41k)
    atol1 = 0.05 * (M ** 0.5)
    assert torch.allclose(s1, yf.sum(0), rtol=2e-2, atol=atol1)
    assert torch.allclose(s2, (yf * yf).sum(0), rtol=2e-2, atol=40 * atol1)
