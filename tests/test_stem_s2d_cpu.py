"""CPU check of the stem's width space-to-depth remapping (conv.py
stem_s2d_input / stem_s2d_weight / stem_s2d_dweight): in float64 the
remapped 8-channel 7x4 stride-(2,1) conv must equal the original 7x7
stride-2 pad-3 conv, and the weight-gradient mapping must round-trip."""

import pytest
import torch
import torch.nn.functional as F

from amdtrain.ops.conv import (stem_s2d_dweight, stem_s2d_input,
                               stem_s2d_weight)

SHAPES = [(2, 32, 32), (1, 20, 28), (1, 14, 6)]


def _remapped_conv(x, w):
    """x [N,3,H,W], w [Cout,3,7,7] -> conv of X' with W2' via F.conv2d."""
    cout = w.shape[0]
    xs = stem_s2d_input(x.permute(0, 2, 3, 1).contiguous())  # [N,H,W/2,8]
    w2 = stem_s2d_weight(w)                         # [Cout, kh, g, p, c]
    xs = xs.permute(0, 3, 1, 2)                     # channels = p*4 + c
    wk = w2.permute(0, 3, 4, 1, 2).reshape(cout, 8, 7, 4)
    # top 3 / bottom 3 rows; left 2 groups, right 1 group (wo = W/2 - 1
    # reaches group W/2)
    xs = F.pad(xs, (2, 1, 3, 3))
    return F.conv2d(xs, wk, stride=(2, 1))


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_s2d_conv_equals_7x7(n, h, w):
    torch.manual_seed(0)
    x = torch.randn(n, 3, h, w, dtype=torch.float64)
    wt = torch.randn(16, 3, 7, 7, dtype=torch.float64)
    ref = F.conv2d(x, wt, stride=2, padding=3)
    got = _remapped_conv(x, wt)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    assert err <= 1e-12, err


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_s2d_input_is_a_reinterpretation(n, h, w):
    """X' rows are the 4-channel-padded NHWC rows taken two at a time."""
    torch.manual_seed(1)
    x = torch.randn(n, h, w, 3, dtype=torch.float64)
    xs = stem_s2d_input(x)
    assert xs.shape == (n, h, w // 2, 8)
    x4 = F.pad(x, (0, 1))
    assert torch.equal(xs.reshape(-1), x4.reshape(-1))


def test_s2d_weight_zero_slots_and_roundtrip():
    torch.manual_seed(2)
    wt = torch.randn(16, 3, 7, 7, dtype=torch.float64)
    w2 = stem_s2d_weight(wt)
    assert w2.shape == (16, 7, 4, 2, 4)
    assert (w2[:, :, 0, 0, :] == 0).all()       # kw = -1
    assert (w2[..., 3] == 0).all()              # padded channel
    assert torch.equal(w2[:, 2, 1, 0, 1], wt[:, 1, 2, 1])   # kw = 2*1+0-1
    assert torch.equal(w2[:, 6, 3, 1, 2], wt[:, 2, 6, 6])   # kw = 2*3+1-1
    back = stem_s2d_dweight(w2.reshape(16, 224), 3)
    assert back.shape == wt.shape
    assert torch.equal(back, wt)


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_s2d_weight_gradient_mapping(n, h, w):
    """d(loss)/dW2' gathered back through stem_s2d_dweight is the original
    conv's weight gradient."""
    torch.manual_seed(3)
    x = torch.randn(n, 3, h, w, dtype=torch.float64)
    wt = torch.randn(8, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    ref = F.conv2d(x, wt, stride=2, padding=3)
    g = torch.randn_like(ref)
    (gref,) = torch.autograd.grad(ref, wt, g)

    w2 = stem_s2d_weight(wt.detach()).requires_grad_(True)
    xs = stem_s2d_input(x.permute(0, 2, 3, 1).contiguous()) \
        .permute(0, 3, 1, 2)
    wk = w2.permute(0, 3, 4, 1, 2).reshape(8, 8, 7, 4)
    y = F.conv2d(F.pad(xs, (2, 1, 3, 3)), wk, stride=(2, 1))
    (g2,) = torch.autograd.grad(y, w2, g)
    got = stem_s2d_dweight(g2.reshape(8, 224), 3)
    err = (got - gref).abs().max().item()
    assert err <= 1e-10 * max(1.0, gref.abs().max().item()), err
