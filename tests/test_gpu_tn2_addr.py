"""GPU check of the incremental gather addressing of the tn2 wgrad kernels
(csrc/wgrad.hip: TnWalk): dW with AMDTRAIN_TN2_ADDR at its default must be
the same bits as with AMDTRAIN_TN2_ADDR=0 (every address derived from m
again), and both must match torch.nn.grad.conv2d_weight in fp32.

With these small M the default split gives every block a single chunk, so
each case also runs with AMDTRAIN_TN2_BLOCKS forcing msplit = 1 (one block
walks every chunk) and forcing two and three parts (blocks start at
mc0 > 0; the parts are uneven wherever the chunk count is not a multiple).
Both switches are read per call."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ext():
    from amdtrain.ops import functional as OF
    assert OF.ext_available()
    return OF.require_ext()


def _nhwc_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _pair(n, cin, cout, h, w, ho, wo, seed):
    torch.manual_seed(seed)
    x = torch.randn(n, cin, h, w, device=DEV).bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    gy = torch.randn(n, cout, ho, wo, device=DEV).bfloat16() \
        .contiguous(memory_format=torch.channels_last)
    return x, gy


def _on_off(monkeypatch, tiles, call, ref):
    """call() under every split, address switch off and on"""
    for blocks in (None, 1, 2 * tiles, 3 * tiles):
        if blocks is None:
            monkeypatch.delenv("AMDTRAIN_TN2_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("AMDTRAIN_TN2_BLOCKS", str(blocks))
        monkeypatch.setenv("AMDTRAIN_TN2_ADDR", "0")
        off = call()
        monkeypatch.delenv("AMDTRAIN_TN2_ADDR")
        on = call()
        assert torch.equal(on, off), \
            (blocks, (on - off).abs().max().item())
        assert torch.allclose(on, ref, atol=0.5, rtol=0.02), \
            (blocks, (on - ref).abs().max().item())
        # the padded-half skip of the N <= 64 tile leaves the bits alone too
        monkeypatch.setenv("AMDTRAIN_TN2_NSKIP", "0")
        full = call()
        monkeypatch.delenv("AMDTRAIN_TN2_NSKIP")
        assert torch.equal(on, full), blocks


# (n, hw, stride, cin, cout, tiles = n-tiles x k-tiles of the config)
CONV3X3 = {
    "s1_crosses_images": (5, 7, 1, 128, 128, 9),     # M = 245
    "s1_two_images_per_chunk_n64": (6, 5, 1, 64, 64, 5),  # M = 150, N = 64
    "s2_odd_input": (4, 15, 2, 128, 128, 9),         # M = 256
    "s2_even_input": (3, 14, 2, 128, 128, 9),        # M = 147
    "s1_deep_k_8wave": (4, 7, 1, 512, 512, 72),      # K9 = 4608, M = 196
    "s1_m_below_64": (1, 7, 1, 128, 128, 9),         # M = 49
    "s1_n64_m_below_64": (2, 5, 1, 64, 64, 5),       # M = 50
    "s1_8wave_m_below_64": (1, 7, 1, 512, 512, 72),  # M = 49
}


@pytest.mark.parametrize("name", sorted(CONV3X3))
def test_conv3x3_walk_equals_direct(name, monkeypatch):
    n, hw, s, cin, cout, tiles = CONV3X3[name]
    e = _ext()
    ho = (hw + 2 - 3) // s + 1
    x, gy = _pair(n, cin, cout, hw, hw, ho, ho, 0)
    x2d, gy2d = _nhwc_rows(x), _nhwc_rows(gy)
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (cout, cin, 3, 3), gy.float(), stride=s, padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(cout, 9 * cin)  # tap-major columns
    _on_off(monkeypatch, tiles,
            lambda: e.tn2_wgrad(gy2d, x2d, 9, n, hw, hw, s, 2), ref)


# (n, hw, stride, channels)
BANDED = {
    "s1": (4, 7, 1, 128),          # M = 196
    "s1_two_groups": (3, 5, 1, 256),  # M = 75, n0 = 128 window
    "s2_odd_input": (2, 15, 2, 128),  # M = 128
    "s1_m_below_64": (1, 7, 1, 128),  # M = 49
}


@pytest.mark.parametrize("name", sorted(BANDED))
def test_banded_walk_equals_direct(name, monkeypatch):
    n, hw, s, ch = BANDED[name]
    e = _ext()
    ho = (hw + 2 - 3) // s + 1
    x, gy = _pair(n, ch, ch, hw, hw, ho, ho, 1)
    x2d, gy2d = _nhwc_rows(x), _nhwc_rows(gy)
    full = torch.nn.grad.conv2d_weight(
        x.float(), (ch, ch, 3, 3), gy.float(), stride=s, padding=1)
    # compact band: row cout keeps its own 128-channel window of every tap
    full = full.permute(0, 2, 3, 1)  # [cout, 3, 3, cin]
    ref = torch.cat([full[g:g + 128, :, :, g:g + 128]
                     for g in range(0, ch, 128)]).reshape(ch, 9 * 128)
    _on_off(monkeypatch, (ch // 128) * 9,
            lambda: e.tn2_wgrad_banded(gy2d, x2d, n, hw, hw, s), ref)


# (n, image size): 7x7 s2 p3 stem, Cin 8 (channel-padded), Cout 64
STEM = {"30x30": (3, 30), "m_below_64": (1, 14)}  # M = 675 / 49


@pytest.mark.parametrize("name", sorted(STEM))
def test_stem_walk_equals_direct(name, monkeypatch):
    n, hw = STEM[name]
    e = _ext()
    ho = (hw + 6 - 7) // 2 + 1
    x, gy = _pair(n, 8, 64, hw, hw, ho, ho, 2)
    x2d, gy2d = _nhwc_rows(x), _nhwc_rows(gy)
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (64, 8, 7, 7), gy.float(), stride=2, padding=3)
    ref = ref.permute(0, 2, 3, 1).reshape(64, 49 * 8)
    _on_off(monkeypatch, 2,  # (1,4,32): K9 = 392 in two 256-wide k-tiles
            lambda: e.tn2_wgrad(gy2d, x2d, 49, n, hw, hw, 2, 2, 7, 7, 3),
            ref)


@pytest.mark.parametrize("name", sorted(STEM))
def test_stem_s2d_walk_equals_direct(name, monkeypatch):
    """the same stem in its width space-to-depth form: 7 x 4 taps, stride
    (2, 1), padding 3 / 2, explicit output dims"""
    from amdtrain.ops.conv import stem_s2d_dweight, stem_s2d_input
    n, hw = STEM[name]
    e = _ext()
    ho = (hw + 6 - 7) // 2 + 1
    x, gy = _pair(n, 3, 64, hw, hw, ho, ho, 2)
    gy2d = _nhwc_rows(gy)
    xs = stem_s2d_input(x.permute(0, 2, 3, 1)).reshape(n * hw * (hw // 2), 8)
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (64, 3, 7, 7), gy.float(), stride=2, padding=3)

    def call():
        return e.tn2_wgrad(gy2d, xs, 28, n, hw, hw // 2, 2, 2, 7, 4, 3,
                           1, 2, ho, ho)

    for blocks in (None, 1, 2, 3):  # one k-tile: tiles = 1
        if blocks is None:
            monkeypatch.delenv("AMDTRAIN_TN2_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("AMDTRAIN_TN2_BLOCKS", str(blocks))
        monkeypatch.setenv("AMDTRAIN_TN2_ADDR", "0")
        off = call()
        monkeypatch.delenv("AMDTRAIN_TN2_ADDR")
        on = call()
        assert torch.equal(on, off), blocks
        dw = stem_s2d_dweight(on, 3)
        assert torch.allclose(dw, ref, atol=0.5, rtol=0.02), \
            (blocks, (dw - ref).abs().max().item())


# (n, hw): strided 1x1, stride 2, 256 -> 128
STRIDED = {
    "14x14": (4, 14),         # M = 196
    "15x15_odd": (4, 15),     # M = 256
    "15x15_chunk_is_image": (3, 15),  # M = 192, Hout*Wout = 64 = MC
    "9x9_ragged": (5, 9),     # M = 125
    "m_below_64": (1, 14),    # M = 49
}


@pytest.mark.parametrize("name", sorted(STRIDED))
def test_strided_walk_equals_direct(name, monkeypatch):
    n, hw = STRIDED[name]
    cin, cout, s = 256, 128, 2
    e = _ext()
    ho = (hw + s - 1) // s
    x, gy = _pair(n, cin, cout, hw, hw, ho, ho, 3)
    x2d, gy2d = _nhwc_rows(x), _nhwc_rows(gy)
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (cout, cin, 1, 1), gy.float(), stride=s).view(cout, cin)
    _on_off(monkeypatch, 2,  # (2,2,64): one n-tile x two k-tiles
            lambda: e.tn2_wgrad(gy2d, x2d, 1, n, hw, hw, s, 1), ref)


def test_strided_n64_walk_equals_direct(monkeypatch):
    """strided 1x1 into 64 channels: the padded dY tile of (2,2,64)"""
    n, hw, cin, cout, s = 3, 10, 256, 64, 2
    e = _ext()
    x, gy = _pair(n, cin, cout, hw, hw, 5, 5, 4)
    x2d, gy2d = _nhwc_rows(x), _nhwc_rows(gy)
    ref = torch.nn.grad.conv2d_weight(
        x.float(), (cout, cin, 1, 1), gy.float(), stride=s).view(cout, cin)
    _on_off(monkeypatch, 2,
            lambda: e.tn2_wgrad(gy2d, x2d, 1, n, hw, hw, s, 1), ref)
