"""The three C-store epilogues of the MFMA kernels (AMDTRAIN_EPILOGUE 0 / 1 /
2, csrc/common.h) must give the same bits: outputs and BN-statistics
partials of modes 1 and 2 are torch.equal to mode 0's on every kernel family
that shares the helper, on interior tiles, ragged edges and the narrow-store
fall-back (N % 8 != 0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available()
    from amdtrain import _C
    return _C


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).bfloat16().to(DEV)


def _same_all_modes(fn):
    """fn(epi) -> tensor or list of tensors; modes 1, 2 equal mode 0"""
    ref = fn(0)
    ref = list(ref) if isinstance(ref, (list, tuple)) else [ref]
    for epi in (1, 2):
        out = fn(epi)
        out = list(out) if isinstance(out, (list, tuple)) else [out]
        assert len(out) == len(ref)
        for k, (a, b) in enumerate(zip(ref, out)):
            assert a.shape == b.shape and a.dtype == b.dtype
            # compare bits: NaN == NaN, -0.0 != 0.0
            bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
            a, b = a.view(bits), b.view(bits)
            assert torch.equal(a, b), f"mode {epi} output {k} differs"
    return ref


@pytest.mark.parametrize("M,N,K", [
    (128, 128, 32),   # one interior tile
    (1, 128, 32),     # single row
    (200, 64, 64),    # ragged M, masked n-waves
    (257, 192, 96),   # half-full last n-tile
    (130, 72, 32),    # N cuts inside a fragment
    (130, 100, 32),   # N % 8 != 0: mode 2 must fall back to narrow stores
])
def test_gemm_bt_modes_equal(M, N, K):
    C = _ext()
    A = _rand((M, K), 1000 + M + N)
    B = _rand((N, K), 2000 + M + N, K ** -0.5)
    ref = _same_all_modes(lambda epi: C.gemm_bt(A, B, False, None, None, epi))
    want = A.float() @ B.float().t()
    assert (ref[0].float() - want).abs().max() <= 2.0 ** -7 * want.abs().max()
    # gemm_bt routes few-tile shapes with K >= 64 to the split-K kernel,
    # which has its own store; the stats entry point always runs the
    # shared epilogue, so the same shapes go through it as well
    y, st = _same_all_modes(lambda epi: C.gemm_bt_stats(A, B, epi))
    assert (y.float() - want).abs().max() <= 2.0 ** -7 * want.abs().max()
    assert st.shape == ((M + 127) // 128, 2 * N)


def test_gemm_bt_signed_zero_and_nan():
    C = _ext()
    M, N, K = 257, 192, 96
    A = _rand((M, K), 7)
    B = _rand((N, K), 8, K ** -0.5)
    A[200] = -0.0              # a row of signed zeros
    A[7, 3] = -0.0
    A[130, 17] = float("nan")  # row 130 of C is NaN
    _same_all_modes(lambda epi: C.gemm_bt(A, B, False, None, None, epi))
    y, st = _same_all_modes(lambda epi: C.gemm_bt_stats(A, B, epi))
    assert torch.isnan(y[130].float()).all()
    assert not torch.isnan(y[129].float()).any()
    assert (y[200].float() == 0).all()
    assert torch.isnan(st[1]).all() and not torch.isnan(st[0]).any()


def test_gemm_bt_stats_plain_modes_equal():
    C = _ext()
    A = _rand((300, 64), 11)
    B = _rand((256, 64), 12, 0.125)
    y, st = _same_all_modes(lambda epi: C.gemm_bt_stats(A, B, epi))
    assert st.shape == (3, 512)
    s1 = y.float().sum(0)  # partials are of the fp32 accumulator, y is bf16
    assert (st[:, :256].sum(0) - s1).abs().max() <= 2.0 ** -8 * 300 * \
        y.float().abs().max()


def test_gemm_bt_stats_n2_modes_equal():
    # dual-n-tile kernel: needs nbm * (nbn / 2) >= 256; 16.8 MB of output
    C = _ext()
    A = _rand((32808, 64), 13)
    B = _rand((256, 64), 14, 0.125)
    y, st = _same_all_modes(lambda epi: C.gemm_bt_stats(A, B, epi))
    assert y.shape == (32808, 256) and st.shape == (257, 512)
    _same_all_modes(lambda epi: C.gemm_bt(A, B, False, None, None, epi))


def test_gemm_bt_strided_modes_equal():
    C = _ext()
    n, h, w = 2, 8, 8
    A = _rand((n * h * w, 64), 15)
    B = _rand((128, 64), 16, 0.125)
    ref = _same_all_modes(
        lambda epi: C.gemm_bt_strided(A, B, n, h, w, 2, epi))
    rows = A.view(n, h, w, 64)[:, ::2, ::2].reshape(-1, 64)
    want = rows.float() @ B.float().t()
    assert ref[0].shape == (n * 16, 128)
    assert (ref[0].float() - want).abs().max() <= 2.0 ** -7 * want.abs().max()


@pytest.mark.parametrize("cout", [64, 128])
def test_conv3x3_fwd_stats_modes_equal(cout):
    C = _ext()
    n, hw, cin = 3, 8, 64   # M = 192: ragged second m-tile
    x = _rand((n * hw * hw, cin), 20 + cout)
    w = _rand((cout, 9 * cin), 30 + cout, (9 * cin) ** -0.5)
    y, st = _same_all_modes(
        lambda epi: C.conv3x3_fwd_stats(x, n, hw, hw, 1, w, False, True, epi))
    assert y.shape == (192, cout) and st.shape == (2, 2 * cout)
    _same_all_modes(lambda epi: C.conv3x3_fwd(x, n, hw, hw, 1, w, True, epi))


@pytest.mark.parametrize("cin", [64, 128])
def test_conv3x3_dgrad_stride1_modes_equal(cin):
    C = _ext()
    n, hw, cout = 3, 8, 64
    gy = _rand((n * hw * hw, cout), 40 + cin)
    w = _rand((cout, 9 * cin), 50 + cin, (9 * cout) ** -0.5)
    _same_all_modes(lambda epi: C.conv3x3_dgrad(gy, n, hw, hw, 1, w, False,
                                                True, True, epi))


@pytest.mark.parametrize("cin", [64, 128])
def test_conv3x3_dgrad_stride2_parity_modes_equal(cin):
    # PAR tiling: 4 classes of 48 rows each (n=3, 8x8 input, 4x4 dy)
    C = _ext()
    n, hw, cout = 3, 8, 64
    gy = _rand((n * 4 * 4, cout), 60 + cin)
    w = _rand((cout, 9 * cin), 70 + cin, (9 * cout) ** -0.5)
    par = _same_all_modes(lambda epi: C.conv3x3_dgrad(
        gy, n, hw, hw, 2, w, False, True, True, epi))
    allt = _same_all_modes(lambda epi: C.conv3x3_dgrad(
        gy, n, hw, hw, 2, w, False, False, True, epi))
    assert torch.equal(par[0], allt[0])


@pytest.mark.parametrize("tile64", [True, False])
def test_stem_fwd_stats_modes_equal(tile64):
    C = _ext()
    n, hw, cout = 2, 32, 64
    x8 = torch.zeros(n * hw * hw, 8, dtype=torch.bfloat16, device=DEV)
    x8[:, :3] = _rand((n * hw * hw, 3), 80)
    w2 = torch.zeros(cout, 416, dtype=torch.bfloat16, device=DEV)
    w2[:, :392] = _rand((cout, 392), 81, 147 ** -0.5)
    y, st = _same_all_modes(lambda epi: C.conv_generic_fwd_stats(
        x8, n, hw, hw, 7, 7, 2, 3, w2, 0, -1, 0, 0, tile64, epi))
    assert y.shape == (n * 16 * 16, cout) and st.shape == (4, 2 * cout)
    _same_all_modes(lambda epi: C.conv_generic_fwd(
        x8, n, hw, hw, 7, 7, 2, 3, w2, 0, -1, 0, 0, tile64, epi))


def test_env_switch_and_default(monkeypatch):
    from amdtrain.ops.conv import _epilogue_mode
    C = _ext()
    monkeypatch.delenv("AMDTRAIN_EPILOGUE", raising=False)
    assert _epilogue_mode() == -1   # each kernel's measured default
    for v in (0, 1, 2):
        monkeypatch.setenv("AMDTRAIN_EPILOGUE", str(v))
        assert _epilogue_mode() == v
    monkeypatch.setenv("AMDTRAIN_EPILOGUE", "3")
    with pytest.raises(ValueError):
        _epilogue_mode()
    # the bindings' own default (no epi argument) is the same -1
    A = _rand((300, 64), 90)
    B = _rand((256, 64), 91, 0.125)
    for a, b in zip(C.gemm_bt_stats(A, B), C.gemm_bt_stats(A, B, 0)):
        assert torch.equal(a, b)
    assert torch.equal(C.gemm_bt(A, B), C.gemm_bt(A, B, False, None, None, 0))
