"""What the level-0 edge tables of tests/pyramid_expected.py cover, asserted without a GPU: every class of the last strip and of the
last segment / tile row under both kernels and both smoothing tap counts, every kernel code of klt_level0_path, frames small enough that
the oracle stays cheap -- and that the comparison the GPU tests rest on notices one ulp."""
import collections

import numpy as np
import pytest

import pyramid_expected as pe
from pyramid_expected import (ALL_CASES, BATCH_SPLIT, COL_CLASSES, MERGED_GRAD, OTHER_PATHS, PYRAMID_SEEDS, RB16, RB32, RB32_HRED, RB32_PLAIN,
                              STREAM, STREAM_CASES, STREAM_NARROW, STREAM_NO_CENTRE, STREAM_ROW_CLASSES, STREAM_WIDE, TILED_HRED_SMALL,
                              TILED_LDS, TILED_ROW_CLASSES, TWO_PASS, case_path, col_class, row_class)

TAPS = {0.1: 5, 0.2: 9}


def test_the_restated_tap_counts():
    """what expected_path takes from the host's tap generator: 5 / 9 / 7 smoothing taps at sigma factors 0.1 / 0.2 / 0.15, 21 reduction
    taps at subsampling 4 only, 7 gradient taps"""
    assert pe._tap_counts(4, 0.1) == (5, 21, 7) and pe._tap_counts(4, 0.2) == (9, 21, 7) and pe._tap_counts(4, 0.15) == (7, 21, 7)
    assert pe._tap_counts(2, 0.1)[1] == 11 and pe._tap_counts(8, 0.2)[1] not in (11, 21)


def test_stream_tables_cover_every_class():
    """every column class and every row class under the streaming kernel, with u8 and with f32 frames (the u8 prefetch and the f32 loads are
    different code: every case runs with both, and streams with both); every row class with 5 and with 9 smoothing taps (the vertical
    halo is rs + 3 rows)"""
    cols, rows = collections.defaultdict(set), collections.defaultdict(set)
    for c in STREAM_CASES:
        for f32 in (False, True):
            assert case_path(c, f32)[0] == (STREAM if f32 else STREAM_NO_CENTRE), c
            cols[col_class(c.ncols)].add(f32)
            rows[row_class(c.nrows)].add((f32, TAPS[c.sigma]))
    assert sorted(cols) == sorted(COL_CLASSES) and all(v == {False, True} for v in cols.values())
    assert sorted(rows) == sorted(STREAM_ROW_CLASSES)
    for name, seen in rows.items():
        assert seen == {(False, 5), (False, 9), (True, 5), (True, 9)}, name


def test_stream_tables_hold_what_the_issue_lists():
    narrow = {(c.ncols, c.nrows % 160) for c in STREAM_NARROW}
    widths = [128, 132, 136, 140, 144, 148, 188, 131, 143, 145, 191, 130, 134, 142, 146, 190]
    rems = [0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 35, 64, 96, 128, 159]
    assert set(zip(widths, rems)) <= narrow
    for c in STREAM_NARROW:
        assert 128 <= c.ncols <= 192 and c.nrows // 160 >= (32 if c.ncols == 128 else 21) and c.batch == 32 and (c.levels, c.ss) == (3, 4)
    one = {c.nrows for c in STREAM_WIDE if c.ncols >= 4096}
    two = {c.nrows for c in STREAM_WIDE if 2048 <= c.ncols < 4096}
    assert one == {64, 65, 67, 96, 97, 159, 160} and two == {161, 163, 167, 192, 193, 320}
    assert {4096, 4100, 4104, 4099} <= {c.ncols for c in STREAM_WIDE}
    # the remainders that had never run: ncols % 4 of 2 and 3, multiples of 4 that are no multiple of 64, last strips inside the halo
    assert {c.ncols % 4 for c in STREAM_CASES} == {0, 1, 2, 3}
    assert any(c.ncols % 4 == 0 and 0 < c.ncols % 64 < 16 for c in STREAM_CASES)


def test_the_streaming_bound():
    """every STREAM_* case streams with the option on and takes the 32-row tile with the reduction with it off; one workgroup fewer in
    the grid would not stream"""
    for c in STREAM_CASES:
        for f32 in (False, True):
            assert case_path(c, f32, 1, 1)[0] in (STREAM, STREAM_NO_CENTRE) and case_path(c, f32, 0, 1)[0] == RB32_HRED
            assert case_path(c, f32, 0, 0)[0] == RB32
    assert pe.expected_path(4096, 64, 31, False, 3, 4, 0.1)[0] == RB32_HRED             # 1984 workgroups
    assert pe.expected_path(127, 10240, 32, False, 3, 4, 0.1)[0] == RB32_HRED           # 4096 workgroups, but a frame of one full strip


def test_frames_stay_small():
    """the point of the tables: batches of small frames, not 1080p"""
    assert all(c.ncols * c.nrows <= 700000 for c in STREAM_CASES)
    assert all(c.ncols * c.nrows < 70000 for c in TILED_HRED_SMALL)
    assert all(c.ncols * c.nrows * c.batch <= 22000000 for c in ALL_CASES)


def test_tiled_tables_cover_every_class():
    cols, rows = collections.defaultdict(set), collections.defaultdict(set)
    for c in TILED_HRED_SMALL:
        for f32 in (False, True):
            if case_path(c, f32)[0] != RB32_HRED:
                continue
            assert case_path(c, f32, 1, 0)[0] == RB32
            cols[col_class(c.ncols)].add(f32)
            rows[row_class(c.nrows, 32)].add((f32, TAPS[c.sigma]))
    assert sorted(cols) == sorted(COL_CLASSES) and all(v == {False, True} for v in cols.values())
    assert sorted(rows) == sorted(TILED_ROW_CLASSES)
    for name, seen in rows.items():
        assert seen == {(False, 5), (False, 9), (True, 5), (True, 9)}, name
    sizes = {(c.ncols, c.nrows) for c in TILED_HRED_SMALL}
    assert {(489, 64), (64, 489), (500, 65), (492, 67), (177, 177), (250, 125), (249, 125)} <= sizes
    assert {c.ncols % 64 for c in TILED_HRED_SMALL} >= {4, 8, 12, 60, 62, 63} and {c.nrows % 32 for c in TILED_HRED_SMALL} >= {0, 1, 3, 7, 8, 31}
    assert 250 * 125 * 32 == 1000000
    short = [c for c in TILED_HRED_SMALL if (c.ncols, c.nrows) == (249, 125)][0]
    assert case_path(short, False) == (RB16, False) and case_path(short, True, 1, 0) == (RB16, False)
    for c in RB32_PLAIN:
        assert case_path(c, False) == (RB32, True) and case_path(c, True) == (RB32, True) and c.ss in (2, 8) and c.levels == 2


def test_grouping_tables():
    want = {(16, 3, 4): (RB32_HRED, True), (17, 3, 4): (RB32_HRED, False), (32, 2, 4): (RB32_HRED, True), (11, 4, 2): (RB16, False),
            (8, 4, 2): (RB16, True)}
    assert {(c.batch, c.levels, c.ss): case_path(c, False) for c in MERGED_GRAD} == want
    assert [c.batch * (c.levels - 1) for c in MERGED_GRAD] == [32, 34, 32, 33, 24]
    split, mixed = BATCH_SPLIT
    assert split.batch == 33 and case_path(split, False) == (RB16, True)               # the query reports the group of one frame ...
    assert pe.expected_path(split.ncols, split.nrows, 32, False, 3, 4, split.sigma)[0] == RB32_HRED      # ... behind a group of 32
    assert mixed.kinds == "mixed" and case_path(mixed, False) == case_path(mixed, True) == (RB32_HRED, True)
    kinds = [f.dtype for f in pe.case_frames(mixed._replace(ncols=70, nrows=66), False)]
    assert kinds == [np.dtype(np.uint8), np.dtype(np.float32)] * 16
    assert [case_path(c, False)[0] for c in OTHER_PATHS] == [TILED_LDS, TWO_PASS]


def _codes(cases):
    n = collections.Counter()
    for c in cases:
        for f32 in (False, True):
            n[case_path(c, f32)[0]] += 1
    return n


def test_every_path_code_is_some_cases_expected_path(capsys):
    n = _codes(ALL_CASES)
    with capsys.disabled():
        print("\ncases per path code (case x dtype): " + ", ".join("%s %d" % (pe.PATH_NAMES[k], n[k]) for k in range(7)))
    assert all(n[k] > 0 for k in (TWO_PASS, TILED_LDS, RB16, RB32, RB32_HRED, STREAM, STREAM_NO_CENTRE))
    assert len({pe.case_id(c) for c in ALL_CASES}) == len(ALL_CASES)                   # (no case twice, unique test ids)


def test_the_draw_table():
    """the 12 fixed seeds of test_gpu_draws.test_pyramid_draw: every path code, merged and separate gradient launches, the size caps"""
    assert len(PYRAMID_SEEDS) == 12
    codes, merged = set(), set()
    for seed in PYRAMID_SEEDS:
        c, f32 = pe.drawn_case(seed)
        assert (c, f32) == pe.drawn_case(seed)
        code, m = case_path(c, f32)
        codes.add(code)
        merged.add(m)
        assert 1 <= c.batch <= 33 and c.ncols * c.nrows * min(c.batch, 32) <= (22000000 if code >= STREAM else 2000000)
        assert c.ncols % 64 in pe.COL_REMAINDERS
        assert c.nrows % 160 in pe.STREAM_ROW_REMAINDERS if code >= STREAM else c.nrows % 32 in pe.TILED_ROW_REMAINDERS
        assert 0 in pe.draw_oracle_frames(c) and all(k < c.batch for k in pe.draw_oracle_frames(c))
    assert codes == set(range(7)) and merged == {False, True}


def test_a_draw_reaches_the_kernel_it_picked():
    seen = collections.Counter()
    for seed in range(100, 160):
        c, f32 = pe.drawn_case(seed)
        seen[case_path(c, f32)[0]] += 1
    assert all(seen[k] > 0 for k in range(7)) and seen[STREAM] + seen[STREAM_NO_CENTRE] >= 10


def test_frames_are_distinct_and_full_range():
    u8 = pe.frames((70, 130), 32, False, 3)
    assert all(f.dtype == np.uint8 and f.min() == 0 and f.max() == 255 for f in u8)
    assert len({f.tobytes() for f in u8}) == 32
    fl = pe.frames((70, 130), 32, True, 3)
    assert len({f.tobytes() for f in fl}) == 32
    for f in fl:
        assert f.dtype == np.float32 and np.isfinite(f).all() and f.min() < -100 and f.max() > 100
        zeros = np.signbit(f) & (f == 0)
        assert zeros[-1, -1] and zeros[:, -1].sum() >= 3 and zeros[-1, :].sum() >= 6 and zeros.sum() > 40
    assert all(np.array_equal(a, b) for a, b in zip(u8, pe.frames((70, 130), 32, False, 3)))


def test_the_oracle_builds_the_smallest_frames():
    """one frame of every TILED_HRED_SMALL, RB32_PLAIN and MERGED_GRAD shape: finite planes of the right sizes down to levels 4 rows high"""
    done = set()
    for c in TILED_HRED_SMALL + RB32_PLAIN + MERGED_GRAD:
        key = (c.ncols, c.nrows, c.levels, c.ss, c.sigma)
        if key in done:
            continue
        done.add(key)
        P = pe.oracle_pyramid(c, pe.frames((c.nrows, c.ncols), 1, False, 1)[0])
        for l in range(c.levels):
            for w in pe.PLANES:
                a = P.level(w, l)
                assert a.shape == (c.nrows // c.ss ** l, c.ncols // c.ss ** l) and np.isfinite(a).all(), (c, w, l)
    c = TILED_HRED_SMALL[0]
    assert (c.ncols, c.nrows) == (489, 64) and [(c.ncols // 4 ** l, c.nrows // 4 ** l) for l in range(3)] == [(489, 64), (122, 16), (30, 4)]


def test_the_comparison_notices_one_ulp():
    a = np.random.default_rng(5).normal(0, 50, (37, 53)).astype(np.float32)
    assert pe.first_difference(a, a.copy()) is None
    b = a.copy()
    b[-1, -1] = np.nextafter(b[-1, -1], np.float32(np.inf))
    bad = pe.first_difference(a, b)
    assert bad is not None and "1 of %d differ" % a.size in bad and "flat index %d " % (a.size - 1) in bad and "(row 36, column 52)" in bad
    z = np.zeros((2, 3), np.float32)
    m = z.copy()
    m[0, 1] = np.float32(-0.0)
    assert "flat index 1 " in pe.first_difference(z, m)                                # +0 against -0: different bits
    n = np.full((2, 2), np.nan, np.float32)
    assert pe.first_difference(n, n.copy()) is None                                    # the same NaN: the same bits
    assert "shape" in pe.first_difference(z, z[:, :2])
