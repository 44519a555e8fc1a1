"""Python mirror of the wide-store C epilogue of the MFMA kernels
(csrc/common.h: epi_col, epi_quad_transpose, epi_store_bf16), checked
against a plain enumeration of a wave's [64][NFRAG*16] sub-tile.

The mirror moves symbolic (row, col) labels through the same two DPP
quad_perm butterfly stages the kernel runs on packed bf16 pairs, so it pins
the B-row map, the v_perm_b32 byte selectors, the select polarity of both
stages, the order of the 8 elements inside a 16-byte run and the row /
column each lane stores it at."""
import pytest

WAVE = 64


def epi_col(j, fr):
    """column of fragment j, lane fr (== LDS B row that lane read)"""
    return (j >> 1) * 32 + (fr >> 2) * 8 + (j & 1) * 4 + (fr & 3)


def _quad_perm(vals, perm):
    """DPP quad_perm: lane l reads lane (l & ~3) + perm[l & 3]"""
    return [vals[(l & ~3) + perm[l & 3]] for l in range(WAVE)]


def _v_perm(s0, s1, sel):
    """v_perm_b32 on dwords of two 16-bit halves (lo, hi): byte pool 0-3 =
    s1, 4-7 = s0; the selectors used only move whole halves."""
    pool = {0: s1[0], 2: s1[1], 4: s0[0], 6: s0[1]}
    lo_b, hi_b = sel & 0xFF, (sel >> 16) & 0xFF
    assert (sel >> 8) & 0xFF == lo_b + 1 and (sel >> 24) & 0xFF == hi_b + 1
    return (pool[lo_b], pool[hi_b])


def quad_transpose(nfrag, acc):
    """acc[lane][j][r] -> run[lane][h] = 8 labels (one 16-byte store)"""
    d = [[[None, None] for _ in range(nfrag)] for _ in range(WAVE)]
    for j in range(nfrag):
        p01 = [(acc[l][j][0], acc[l][j][1]) for l in range(WAVE)]
        p23 = [(acc[l][j][2], acc[l][j][3]) for l in range(WAVE)]
        x01 = _quad_perm(p01, (1, 0, 3, 2))
        x23 = _quad_perm(p23, (1, 0, 3, 2))
        sel = [0x03020706 if (l & 1) else 0x05040100 for l in range(WAVE)]
        q01 = [_v_perm(x01[l], p01[l], sel[l]) for l in range(WAVE)]
        q23 = [_v_perm(x23[l], p23[l], sel[l]) for l in range(WAVE)]
        low = [not (l & 2) for l in range(WAVE)]
        send = [q23[l] if low[l] else q01[l] for l in range(WAVE)]
        recv = _quad_perm(send, (2, 3, 0, 1))
        for l in range(WAVE):
            d[l][j][0] = q01[l] if low[l] else recv[l]
            d[l][j][1] = recv[l] if low[l] else q23[l]
    run = [[None] * (nfrag // 2) for _ in range(WAVE)]
    for l in range(WAVE):
        for h in range(nfrag // 2):
            dwords = (d[l][2 * h][0], d[l][2 * h][1],
                      d[l][2 * h + 1][0], d[l][2 * h + 1][1])
            run[l][h] = [half for dw in dwords for half in dw]
    return run


def wave_stores(nfrag, i, out):
    """mirror of the WIDE branch of epi_store_bf16 for m-fragment i: list of
    wave store instructions, each [(row, col0, 8 labels)] by lane"""
    return [[(i * 16 + (l >> 4) * 4 + (l & 3),
              h * 32 + ((l & 15) >> 2) * 8, out[l][h]) for l in range(WAVE)]
            for h in range(nfrag // 2)]


def lane_runs(nfrag):
    """per lane and m-fragment, what epi_quad_transpose leaves: (row, col0)
    of each 32-column group h, rows/cols local to the wave tile"""
    out = {}
    for lane in range(WAVE):
        fr, fq = lane & 15, lane >> 4
        out[lane] = [(i * 16 + fq * 4 + (fr & 3), h * 32 + (fr >> 2) * 8)
                     for i in range(4) for h in range(nfrag // 2)]
    return out


@pytest.mark.parametrize("nfrag", [4, 2])
def test_col_map_is_a_bijection_of_the_wave_span(nfrag):
    cols = sorted(epi_col(j, fr) for j in range(nfrag) for fr in range(16))
    assert cols == list(range(nfrag * 16))


@pytest.mark.parametrize("nfrag", [4, 2])
def test_transpose_gives_each_lane_contiguous_aligned_runs(nfrag):
    span = nfrag * 16
    runs = lane_runs(nfrag)
    covered = set()
    for i in range(4):
        # MFMA C layout: lane holds rows fq*4 + r of one column per fragment
        acc = [[[(i * 16 + (l >> 4) * 4 + r, epi_col(j, l & 15))
                 for r in range(4)] for j in range(nfrag)]
               for l in range(WAVE)]
        out = quad_transpose(nfrag, acc)
        for lane in range(WAVE):
            for h in range(nfrag // 2):
                row, col0 = runs[lane][i * (nfrag // 2) + h]
                # one row, 8 consecutive columns in address order
                assert out[lane][h] == [(row, col0 + k) for k in range(8)]
                # 16-byte aligned whenever the row pitch is (N % 8 == 0)
                assert col0 % 8 == 0 and col0 + 8 <= span
                covered.update(out[lane][h])
    # every element of the plain 64 x span enumeration, exactly once
    assert covered == {(r, c) for r in range(64) for c in range(span)}
    assert sum(len(v) for v in runs.values()) * 8 == 64 * span


@pytest.mark.parametrize("nfrag", [4, 2])
def test_wave_stores_land_where_the_labels_say(nfrag):
    """the address each lane stores a run at is the run's own (row, col0);
    all stores together cover the tile once; one instruction writes 64
    contiguous bytes of each of 16 rows"""
    span = nfrag * 16
    covered = []
    n_ins = 0
    for i in range(4):
        acc = [[[(i * 16 + (l >> 4) * 4 + r, epi_col(j, l & 15))
                 for r in range(4)] for j in range(nfrag)]
               for l in range(WAVE)]
        for ins in wave_stores(nfrag, i, quad_transpose(nfrag, acc)):
            n_ins += 1
            by_row = {}
            for row, col0, labels in ins:
                assert labels == [(row, col0 + k) for k in range(8)]
                assert col0 % 8 == 0
                by_row.setdefault(row, []).append(col0)
                covered += labels
            assert len(by_row) == 16
            for cols in by_row.values():
                cols.sort()
                assert [c - cols[0] for c in cols] == [0, 8, 16, 24]
    assert n_ins == 2 * nfrag  # 8 per 64x64 wave tile (was 64 2-byte ones)
    assert sorted(covered) == [(r, c) for r in range(64) for c in range(span)]


@pytest.mark.parametrize("nfrag", [4, 2])
def test_stats_label_is_the_b_row_read(nfrag):
    """epilogue_stats sums fragment j of lane fr over rows and files it under
    wn + epi_col(j, fr): that must be the B row the lane's MFMA operand came
    from, and after the reduction every column is written exactly once."""
    wn = nfrag * 16  # the second n-wave
    label = {(j, fr): wn + epi_col(j, fr)  # == the LDS B row index read
             for j in range(nfrag) for fr in range(16)}
    assert sorted(label.values()) == list(range(wn, wn + nfrag * 16))
    # the column a lane accumulates is the column its stored elements carry
    acc = [[[((l >> 4) * 4 + r, epi_col(j, l & 15)) for r in range(4)]
            for j in range(nfrag)] for l in range(WAVE)]
    for l in range(WAVE):
        for j in range(nfrag):
            assert {c for _, c in acc[l][j]} == {label[(j, l & 15)] - wn}
