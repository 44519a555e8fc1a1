"""Routing of the pointwise GEMM on the 8 grid and the MobileNetV2 width
multipliers, checked without a GPU."""
import pytest
import torch
import torch.nn as nn

from amdtrain.models import build_model, model_names
from amdtrain.ops.conv import pw_thin_ok, pw_wide_ok

WIDE_140 = {(192, 48), (48, 288), (288, 48), (288, 88), (88, 528), (528, 88),
            (528, 136), (136, 816), (816, 136), (816, 224)}
WIDTHS = {  # stem, the seven stages, head
    "mobilenet_v2_140": [48, 24, 32, 48, 88, 136, 224, 448, 1792],
    "mobilenet_v2_075": [24, 16, 24, 24, 48, 72, 120, 240, 1280],
    "mobilenet_v2_050": [16, 8, 16, 16, 32, 48, 80, 160, 1280],
}


def test_predicate():
    for cin in range(8, 1025, 8):
        for cout in range(8, 1025, 8):
            # symmetric, and exactly what the 32 grid and the thin kernel leave
            assert pw_wide_ok(cin, cout) == pw_wide_ok(cout, cin) \
                == (not (cin % 32 == 0 and cout % 32 == 0)
                    and not pw_thin_ok(cin, cout))
    for pair in [(44, 240), (240, 44), (480, 84), (12, 24), (0, 48), (48, 0)]:
        assert not pw_wide_ok(*pair)
    assert all(pw_wide_ok(*p) for p in WIDE_140 | {(480, 80), (40, 240)})


@pytest.mark.parametrize("arch", sorted(WIDTHS))
def test_width_variants(arch):
    assert arch in model_names()
    m = build_model(arch).eval()
    f = m.features
    assert [f[0][0].out_channels] \
        + [f[i].conv[-2].out_channels for i in (1, 2, 4, 7, 11, 14, 17)] \
        + [f[18][0].out_channels] == WIDTHS[arch]
    assert len(m.state_dict()) == 314
    with torch.no_grad():
        assert tuple(m(torch.randn(2, 3, 32, 32)).shape) == (2, 1000)


def test_routes_of_width_140_and_width_one():
    pairs = {(c.in_channels, c.out_channels)
             for c in build_model("mobilenet_v2_140").modules()
             if isinstance(c, nn.Conv2d) and c.kernel_size == (1, 1)}
    assert {p for p in pairs if pw_wide_ok(*p)} == WIDE_140
    m = build_model("mobilenet_v2", width_mult=1.0, round_nearest=8)
    assert sum(p.numel() for p in m.parameters()) == 3_504_872
