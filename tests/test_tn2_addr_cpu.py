"""Python mirror of the incremental gather addressing of the tn2 wgrad
kernels (csrc/wgrad.hip: tn2_make_step, TnWalk, tn2_range_mask), checked
against the direct formulas it replaces (tn2_decode_row + tn2_gather_tap,
tn2_gather_stride).

The mirror walks a row slot the way a thread does: decode (n, ho, wo) once at
the block's first chunk, then advance by MC rows per chunk with the
precomputed steps and two carries, keeping the tap-0 pixel (hb, wb), its byte
address and the kh / kw validity mask.  Columns carry a loop-invariant byte
offset and the two mask bits they need.  Every staged 16-byte unit of every
chunk must read the byte the direct formulas name, or the zero page."""
import numpy as np
import pytest

NEVER = 0x80000000
ZERO_PAGE = -1


class Geom:
    def __init__(self, H, W, kh=3, kw=3, stride=1, pad=1, sw=None, pw=None,
                 Hout=None, Wout=None):
        self.H, self.W, self.kh, self.kw = H, W, kh, kw
        self.stride, self.pad = stride, pad
        self.sw = stride if sw is None else sw
        self.pw = pad if pw is None else pw
        self.Hout = (H + 2 * pad - kh) // stride + 1 if Hout is None else Hout
        self.Wout = ((W + 2 * self.pw - kw) // self.sw + 1
                     if Wout is None else Wout)


def strided_geom(H, W, s):
    """the geometry tn2_wgrad builds for gmode 1"""
    return Geom(H, W, 1, 1, s, 0, s, 0, (H + s - 1) // s, (W + s - 1) // s)


# ---- mirror ----------------------------------------------------------------

def make_step(g, MC, ld):
    """tn2_make_step"""
    hw = g.Hout * g.Wout
    dn, rem = MC // hw, MC % hw
    dh, dw = rem // g.Wout, rem % g.Wout
    st = dict(
        step=(dn * g.H * g.W + dh * g.stride * g.W + dw * g.sw) * ld * 2,
        cw=(g.stride * g.W - g.Wout * g.sw) * ld * 2,
        ch=(g.H * g.W - g.Hout * g.stride * g.W) * ld * 2,
        dhb=dh * g.stride, dwb=dw * g.sw,
        hhi=g.Hout * g.stride - g.pad, whi=g.Wout * g.sw - g.pw,
        hspan=g.Hout * g.stride, wspan=g.Wout * g.sw)
    assert all(abs(st[k]) < 1 << 29 for k in ("step", "cw", "ch"))
    assert max(g.kh, g.kw, g.pad, g.pw) <= 15
    return st


def range_mask(b, size, k):
    """tn2_range_mask: bits t of [0, k) with 0 <= b + t < size"""
    lo = max(-b, 0)
    hi = max(min(size - b, k), lo)
    return (1 << hi) - (1 << lo)


def walk_rows(g, mode, MC, ld, M, mc0, mc1):
    """base byte offset (X = 0) and mask of every row of chunks mc0..mc1-1,
    each row slot decoded once at mc0 and then stepped"""
    st = make_step(g, MC, ld)
    rows = (mc1 - mc0) * MC
    base = np.zeros(rows, dtype=np.int64)
    mask = np.zeros(rows, dtype=np.int64)
    for r in range(MC):  # a (row slot, lane) pair of the block
        m = mc0 * MC + r
        wo, t = m % g.Wout, m // g.Wout
        ho, n = t % g.Hout, t // g.Hout
        hb, wb = ho * g.stride - g.pad, wo * g.sw - g.pw
        b = ((n * g.H + hb) * g.W + wb) * ld * 2
        for ch in range(mc1 - mc0):
            assert -g.pad <= hb < st["hhi"] and -g.pw <= wb < st["whi"]
            inside = 1 if mode == 1 else (
                range_mask(hb, g.H, g.kh) | range_mask(wb, g.W, g.kw) << 16)
            base[ch * MC + r] = b
            mask[ch * MC + r] = inside if m < M else 0
            m += MC
            wb += st["dwb"]
            c1 = wb >= st["whi"]
            wb -= st["wspan"] if c1 else 0
            hb += st["dhb"] + (g.stride if c1 else 0)
            c2 = hb >= st["hhi"]
            hb -= st["hspan"] if c2 else 0
            b += st["step"] + (st["cw"] if c1 else 0) + (st["ch"] if c2 else 0)
    return base, mask


def column_consts(g, mode, cin, ld, col0, ncols, total_cols):
    """toff / sel of the 16-byte units of a k-tile"""
    cols = np.arange(col0, col0 + ncols, 8)
    toff = np.zeros(len(cols), dtype=np.int64)
    sel = np.zeros(len(cols), dtype=np.int64)
    for i, col in enumerate(cols):
        inr = col + 8 <= total_cols
        if mode == 1:
            toff[i], sel[i] = col * 2, 1 if inr else NEVER
        else:
            tap = col // cin
            kh, kw = tap // g.kw, tap % g.kw
            toff[i] = ((kh * g.W + kw) * ld + (col - tap * cin)) * 2
            sel[i] = ((1 << (kh & 15)) | (0x10000 << (kw & 15))) if inr \
                else NEVER
    return cols, toff, sel


def walk_units(g, mode, MC, cin, M, mc0, mc1, col0, ncols, total_cols):
    base, mask = walk_rows(g, mode, MC, cin, M, mc0, mc1)
    cols, toff, sel = column_consts(g, mode, cin, cin, col0, ncols,
                                    total_cols)
    ok = (mask[:, None] & sel[None, :]) == sel[None, :]
    return np.where(ok, base[:, None] + toff[None, :], ZERO_PAGE)


# ---- the direct formulas ---------------------------------------------------

def direct_units(g, mode, MC, cin, M, mc0, mc1, col0, ncols, total_cols):
    m = np.arange(mc0 * MC, mc1 * MC, dtype=np.int64)[:, None]
    col = np.arange(col0, col0 + ncols, 8, dtype=np.int64)[None, :]
    live = (m < M) & (col + 8 <= total_cols)
    mm = np.minimum(m, M - 1)
    wo, t = mm % g.Wout, mm // g.Wout
    ho, n = t % g.Hout, t // g.Hout
    if mode == 1:  # tn2_gather_stride
        row = (n * g.H + ho * g.stride) * g.W + wo * g.stride
        return np.where(live, (row * cin + col) * 2, ZERO_PAGE)
    tap = col // cin
    kh = tap // g.kw
    h = ho * g.stride - g.pad + kh
    w = wo * g.sw - g.pw + tap - kh * g.kw
    live = live & (h >= 0) & (h < g.H) & (w >= 0) & (w < g.W)
    row = (n * g.H + h) * g.W + w
    return np.where(live, (row * cin + (col - tap * cin)) * 2, ZERO_PAGE)


def check(g, mode, MC, cin, nimg, ncols_tile=128):
    M = nimg * g.Hout * g.Wout
    taps = 1 if mode == 1 else g.kh * g.kw
    total = taps * cin
    mchunks = (M + MC - 1) // MC
    # the whole range from chunk 0, and blocks of an uneven split that
    # start at mc0 > 0 (the last one ends in the ragged chunk)
    spans = {(0, mchunks)}
    for msplit in (2, 3):
        cpp = (mchunks + msplit - 1) // msplit
        for p in range(1, msplit):
            if p * cpp < mchunks:
                spans.add((p * cpp, min((p + 1) * cpp, mchunks)))
    # every k-tile, the last one reaching past the last tap
    ncols = (total + ncols_tile - 1) // ncols_tile * ncols_tile
    for mc0, mc1 in sorted(spans):
        got = walk_units(g, mode, MC, cin, M, mc0, mc1, 0, ncols, total)
        want = direct_units(g, mode, MC, cin, M, mc0, mc1, 0, ncols, total)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (mc0, mc1, bad[:4].tolist(),
                               got[tuple(bad[0])], want[tuple(bad[0])])
    # in range: every live unit's 16 bytes lie inside X
    live = got[got != ZERO_PAGE]
    assert live.min() >= 0 and live.max() + 16 <= nimg * g.H * g.W * cin * 2


# Hout*Wout of 1, 25, 49, 64, 225, 1024 and 12544; Wout below, equal to and
# above MC; stride 1 and 2 on odd and even inputs; non-square images
CONV_GEOMS = {
    "1x1img": (Geom(1, 1), 8, 70),
    "5x5": (Geom(5, 5), 16, 6),
    "7x7": (Geom(7, 7), 16, 5),
    "8x8": (Geom(8, 8), 8, 3),
    "15x15": (Geom(15, 15), 8, 3),
    "15to8_s2": (Geom(15, 15, stride=2), 16, 4),
    "16to8_s2": (Geom(16, 16, stride=2), 8, 3),
    "14to7_s2": (Geom(14, 14, stride=2), 8, 5),
    "3x32": (Geom(3, 32), 8, 3),
    "2x64": (Geom(2, 64), 8, 3),
    "5x72": (Geom(5, 72), 8, 2),
    "32x32": (Geom(32, 32), 8, 2),
    "stem_7x7_s2_p3_30": (Geom(30, 30, 7, 7, 2, 3), 8, 3),
    "stem_7x7_s2_p3_224": (Geom(224, 224, 7, 7, 2, 3), 8, 1),
    "stem_s2d_30": (Geom(30, 15, 7, 4, 2, 3, 1, 2, 15, 15), 8, 3),
    "stem_s2d_224": (Geom(224, 112, 7, 4, 2, 3, 1, 2, 112, 112), 8, 1),
    "5x5_filter_p2": (Geom(9, 11, 5, 5, 1, 2), 8, 2),
}


@pytest.mark.parametrize("MC", [32, 64])
@pytest.mark.parametrize("name", sorted(CONV_GEOMS))
def test_tap_gather_walk(name, MC):
    g, cin, nimg = CONV_GEOMS[name]
    check(g, 2, MC, cin, nimg, ncols_tile=256 if MC == 32 else 128)


def test_tap_gather_walk_banded_window():
    """BAND: the k-tile is one tap's 128-channel window at col0 = tap*Cin +
    n0 of a wider Cin"""
    g, cin, nimg, MC = Geom(7, 7), 256, 4, 64
    M = nimg * 49
    mch = (M + MC - 1) // MC
    for tap in range(9):
        for n0 in (0, 128):
            col0 = tap * cin + n0
            got = walk_units(g, 2, MC, cin, M, 1, mch, col0, 128, 9 * cin)
            want = direct_units(g, 2, MC, cin, M, 1, mch, col0, 128, 9 * cin)
            assert np.array_equal(got, want), (tap, n0)


STRIDED_GEOMS = {
    "2to1": (strided_geom(2, 2, 2), 70),
    "14to7": (strided_geom(14, 14, 2), 4),
    "15to8": (strided_geom(15, 15, 2), 4),
    "9x13_s2": (strided_geom(9, 13, 2), 3),
    "64to32": (strided_geom(64, 64, 2), 2),
    "4x128_s2": (strided_geom(4, 128, 2), 3),
    "224to112": (strided_geom(224, 224, 2), 1),
    "10to4_s3": (strided_geom(10, 10, 3), 5),
}


@pytest.mark.parametrize("MC", [32, 64])
@pytest.mark.parametrize("name", sorted(STRIDED_GEOMS))
def test_strided_walk(name, MC):
    g, nimg = STRIDED_GEOMS[name]
    check(g, 1, MC, 24, nimg)


def test_range_mask_enumerated():
    for size in (1, 2, 5, 30):
        for k in (1, 3, 4, 7, 15):
            for b in range(-15, size + 20):
                want = sum(1 << t for t in range(k) if 0 <= b + t < size)
                assert range_mask(b, size, k) == want, (b, size, k)
