"""What the selection score tables of tests/select_scores_expected.py cover, asserted without a GPU: every class of tile, band and strip
edge named there, on a row or column that some window reads; every klt_select_score_path code; frames within the pixel cap whose oracle
maps put at least a tenth of their values on either side of the case's threshold; the key layout; and that the comparisons the GPU tests
rest on notice one ulp of one value and one key flipped between zero and non-zero."""
import collections

import numpy as np

import select_scores_expected as se
from select_scores_expected import (ALL_CASES, BARRIER, COLS_PIPE, FUSED, ROWS_PIPE, SORTED, case_path, expected, read_extent)


def _reached(values, wanted, what):
    assert set(wanted) <= set(values), "%s: %s never occur" % (what, sorted(set(wanted) - set(values)))


def test_expected_score_path_restates_the_host():
    f = se.expected_score_path
    assert f(128, 64, 7, 7, 4, 4, 0, 1, False) == (1, 1) and f(128, 64, 7, 7, 4, 4, 0, 1, True) == (1, 2)
    assert f(128, 64, 7, 7, 4, 4, 0, 0, True) == (0, 0) and f(128, 64, 7, 7, 4, 4, 0, 0, False) == (0, 0)
    for nc in (129, 130, 131):                                      # the silent fallback: barrier rows, and the fused kernel still applies
        assert f(nc, 64, 7, 7, 4, 4, 0, 1, False) == (0, 0) and f(nc, 64, 7, 7, 4, 4, 0, 1, True) == (0, 2)
    assert f(128, 64, 23, 23, 12, 12, 0, 1, True) == (1, 2) and f(128, 64, 25, 25, 13, 13, 0, 1, True) == (1, 1)      # 9 and 7 columns per strip
    assert f(128, 64, 7, 7, 4, 4, 1, 1, True) == (1, 1) and f(128, 64, 7, 7, 4, 4, 2, 1, True) == (1, 1)
    assert not se.fused_ok(128, 64, 7, 33, 4, 17, 0) and se.fused_ok(128, 64, 7, 31, 4, 16, 0)                       # a window taller than a tile
    assert not se.fused_ok(8, 64, 7, 7, 4, 4, 0)                                                                      # no candidates


def test_every_frame_is_within_the_pixel_cap_and_ids_are_unique():
    assert all(c.ncols * c.nrows <= se.MAX_PIXELS for c in ALL_CASES)
    assert all(c.ncols * c.nrows <= se.MAX_PIXELS for c in map(se.draw_scores, se.SCORES_SEEDS))
    assert len({se.case_id(c) for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        bx, by = se.borders(c)
        hw, hh, step, nx, ny = se.geometry(c)
        assert nx > 0 and ny > 0 and bx >= hw + 1 and by >= hh + 1 and c.ww == c.wh and 3 <= c.ww <= 31, c
        if c.table != "BARRIER" and c.bx is None and c.skip == 0:
            assert read_extent(c) == (c.ncols - 1, c.nrows - 1)        # the smallest border: the last row and column read are n - 2


def test_rows_pipe_table():
    cl = [se.rows_pipe_class(c) for c in ROWS_PIPE]
    _reached([k[0] for k in cl], se.ROWS_PIPE_TILES, "128-column tiles per row")
    _reached([k[1] for k in cl], se.ROWS_PIPE_WIDTHS, "last tile width")
    _reached([k[2] for k in cl], se.ROWS_PIPE_ROWMODS, "rows read mod 16")
    assert any(k[3] for k in cl) and {k[4] for k in cl} == {0, 1}      # a frame of fewer than 16 rows; odd and even row counts
    for c in ROWS_PIPE:
        C = read_extent(c)[0]
        assert c.ncols % 4 == 0 and case_path(c, 1, False) == (1, 1) and case_path(c, 0, False) == (0, 0)
        assert (C - 1) // se.RT == (c.ncols - 1) // se.RT               # the last column read lies in the frame's last tile ...
        assert (C - 1) % se.RT // 64 == (c.ncols - 1) % se.RT // 64     # ... and in its last half-tile (a loader lane's second pixel pair)
        assert C - 1 == c.ncols - 2                                     # ... and is the column the loads are clamped to


def test_cols_pipe_table():
    cl = [se.cols_pipe_class(c) for c in COLS_PIPE]
    _reached([k[0] for k in cl], se.COLS_PIPE_WIDTHS, "ncols % 64")
    _reached([k[1] for k in cl], se.COLS_PIPE_TILES, "64-row tiles per column")
    _reached([k[2] for k in cl], se.COLS_PIPE_ROWMODS, "rows read mod 64")
    for c in COLS_PIPE:
        C = read_extent(c)[0]
        assert c.ncols % 4 == 0 and case_path(c, 1, False) == (1, 1)
        assert (C - 1) // se.CS == (c.ncols - 1) // se.CS and C - 1 >= c.ncols - 4      # the last strip, and the quad the loads are clamped to, are read


def test_barrier_table():
    cl = [se.barrier_class(c) for c in BARRIER]
    for k, (wanted, what) in enumerate([(se.BARRIER_COL_TILES, "64-column tiles"), (se.BARRIER_COL_MODS, "columns read mod 64"),
                                        (se.BARRIER_ROW_TILES, "32-row tiles"), (se.BARRIER_ROW_MODS32, "rows read mod 32"),
                                        (se.BARRIER_ROW_MODS16, "rows read mod 16")]):
        _reached([v[k] for v in cl], wanted, what)
    assert {c.ncols % 4 for c in BARRIER} == {0, 1, 2, 3}
    for c in BARRIER:
        assert case_path(c, 0, False) == (0, 0) and case_path(c, 0, True) == (0, 0)
        assert case_path(c, 1, False) == ((1, 1) if c.ncols % 4 == 0 else (0, 0))      # the fallback that the path code must report
    # below, at, one above and two turns of the register rings
    assert se.SR_D in se.BARRIER_COL_TILES and se.SR_D + 1 in se.BARRIER_COL_TILES and 2 * se.SR_D + 1 in se.BARRIER_COL_TILES
    assert se.SC_D in se.BARRIER_ROW_TILES and se.SC_D + 1 in se.BARRIER_ROW_TILES and 2 * se.SC_D + 1 in se.BARRIER_ROW_TILES


def test_fused_table():
    fused = [c for c in FUSED if case_path(c)[1] == se.FUSED_KEYS]
    cl = [se.fused_class(c) for c in fused]
    for k, (wanted, what) in enumerate([(se.FUSED_PER, "candidate columns per strip"), (se.FUSED_KINDS, "nx against a strip"),
                                        (se.FUSED_TILES, "32-row tiles"), (se.FUSED_ROWMODS, "rows read mod 32"),
                                        (se.FUSED_FIRST, "first scored tile"), (se.FUSED_C0, "first strip's start column mod 4")]):
        _reached([v[k] for v in cl], wanted, what)
    for per in se.FUSED_PER:                                            # every window width with every relation of nx to a strip
        assert {v[1] for v in cl if v[0] == per} >= set(se.FUSED_KINDS), per
    assert {c.thr for c in fused} == set(se.THRESHOLDS)
    assert {case_path(c) for c in fused} == {(1, 2), (0, 2)}
    declined = [c for c in FUSED if case_path(c)[1] != se.FUSED_KEYS]
    assert {(c.ww, c.skip) for c in declined} == {(25, 0), (31, 0), (7, 1), (7, 2)} and all(case_path(c) == (1, 1) for c in declined)
    assert all(c.twice for c in FUSED)
    both = 0
    for c in fused:                                                     # a window's top row in the tile before its bottom row, and in the same tile
        hh = c.wh // 2
        bottoms = np.arange(se.borders(c)[1], se.borders(c)[1] + se.geometry(c)[4]) + hh
        before = (bottoms - 2 * hh - 1) // se.FT < bottoms // se.FT
        both += bool(before.any() and not before.all())
        big = se.other_frame(c)
        assert big.shape[0] > c.nrows and big.shape[1] > c.ncols and big.size <= 2 * se.MAX_PIXELS
    assert both >= 12                                                   # (cases of one scored tile have no row before it)


def test_sorted_table():
    counts = sorted(se.geometry(c)[3] * se.geometry(c)[4] for c in SORTED)
    assert counts[:6] == [2047, 2048, 2049, 4095, 4096, 4097] and 8193 <= counts[6] <= 16384
    assert all(c.sorted for c in SORTED) and not any(c.sorted for c in ROWS_PIPE + COLS_PIPE + BARRIER + FUSED)


def test_every_path_code_is_reached(capsys):
    n = collections.Counter()
    for c in ALL_CASES:
        for variant in (1, 0):
            for prepared in (False, True):
                n[case_path(c, variant, prepared)] += 1
    with capsys.disabled():
        print("\nruns per path code (case x variant x prepared): " + ", ".join("%s %d" % (se.PATH_NAMES[k], n[k]) for k in sorted(n)))
    assert set(n) == {(0, 0), (1, 1), (1, 2), (0, 2)}
    assert {case_path(se.draw_scores(s)) for s in se.SCORES_SEEDS} == {(0, 0), (1, 1), (1, 2), (0, 2)}
    assert all(se.draw_scores(s) == se.draw_scores(s) for s in se.SCORES_SEEDS)


def test_a_draw_reaches_the_path_it_picked():
    seen = collections.Counter(case_path(se.draw_scores(s)) for s in range(100, 140))
    assert all(seen[k] > 0 for k in [(0, 0), (1, 1), (1, 2), (0, 2)])


def test_both_sides_of_every_threshold():
    """at least a tenth of every frame's map on either side of the case's threshold, so that both branches of the compare run; an exact
    threshold really has a map value on the boundary"""
    for c in ALL_CASES + [se.draw_scores(s) for s in se.SCORES_SEEDS]:
        e = expected(c)
        below, kept = se.threshold_split(e)
        assert below >= 0.1 and kept >= 0.1, (se.case_id(c), below, kept)
        wide = e.val.astype(np.float64)
        if c.thr == "at":
            assert (wide == e.min_eig).any() and e.min_eig > 1 and np.all(e.keys[wide == e.min_eig] != 0)
        elif c.thr == "above":
            on = np.nextafter(wide, np.inf) == e.min_eig
            assert on.any() and np.all(e.keys[on] == 0) and np.float32(e.min_eig) == e.val[on][0]      # rounding the threshold to f32 would keep it
        elif c.thr == "frac":
            assert np.float64(np.float32(e.min_eig)) != e.min_eig                                     # no f32 value
        else:
            assert e.min_eig == 1.0
    assert len({expected(c).frame.tobytes() for c in ALL_CASES}) == len(ALL_CASES)                    # distinct textures
    c = FUSED[5]
    assert not np.array_equal(se.other_frame(c)[:c.nrows, :c.ncols], expected(c).frame)


def test_the_key_layout_round_trips():
    """bits(v) << 32 | x << 16 | y, as klt_key_val / klt_key_x / klt_key_y (klt_internal.h) take it apart"""
    val = np.array([[1.0, 0.5, 3.25], [np.float32(1e9), 1.0000001, 0.99999994]], np.float32)
    xs, ys = np.array([2, 65535, 300]), np.array([7, 65534])
    keys = se.pack_keys(val, xs, ys, 0.0)
    assert keys.dtype == np.uint64 and keys[0, 0] == (0x3f800000 << 32) | (2 << 16) | 7
    keep = keys != 0
    assert keep.tolist() == [[True, False, True], [True, True, False]]                       # the floor is max(min_eigenvalue, 1)
    assert np.array_equal(se.key_val(keys[keep]).view(np.uint32), val[keep].view(np.uint32))
    assert np.array_equal(se.key_x(keys[keep]), np.broadcast_to(xs[None, :], val.shape)[keep])
    assert np.array_equal(se.key_y(keys[keep]), np.broadcast_to(ys[:, None], val.shape)[keep])
    assert np.all(np.diff(np.sort(keys[keep])) > 0)
    # u64 order is (val, x, y) order
    a, b, c = se.pack_keys(np.array([[2.0]], np.float32), [5], [9], 1), se.pack_keys(np.array([[2.0]], np.float32), [6], [1], 1), se.pack_keys(np.array([[2.5]], np.float32), [0], [0], 1)
    assert a[0, 0] < b[0, 0] < c[0, 0]


def test_the_comparisons_notice_one_ulp_and_one_flipped_key():
    c = FUSED[6]
    e = expected(c)
    assert se.first_map_difference(c, e.val.copy(), e.val, e.xs, e.ys) is None
    assert se.first_key_difference(c, e.keys.copy(), e.keys, e.xs, e.ys) is None
    v = e.val.copy()
    j, i = v.shape[0] - 1, v.shape[1] - 1
    v[j, i] = np.nextafter(v[j, i], np.float32(np.inf))
    bad = se.first_map_difference(c, v, e.val, e.xs, e.ys)
    assert bad and "1 of %d values differ" % v.size in bad and "pixel (x %d, y %d)" % (e.xs[i], e.ys[j]) in bad and "fused: strip" in bad
    k = e.keys.copy()
    j, i = (int(t) for t in np.argwhere(k != 0)[0])
    k[j, i] = 0                                                         # a kept key dropped
    bad = se.first_key_difference(c, k, e.keys, e.xs, e.ys)
    assert bad and "1 of %d keys differ" % k.size in bad and "got 0x0000000000000000" in bad
    k = e.keys.copy()
    j, i = (int(t) for t in np.argwhere(k == 0)[-1])
    k[j, i] = se.pack_keys(e.val[j:j + 1, i:i + 1], e.xs[i:i + 1], e.ys[j:j + 1], 0.0)[0, 0] or 1      # a dropped key kept
    bad = se.first_key_difference(c, k, e.keys, e.xs, e.ys)
    assert bad and "1 of %d keys differ" % k.size in bad and "want 0x0000000000000000" in bad
    k = e.keys.copy()
    k[0, 0] ^= np.uint64(1 << 32)                                       # one ulp of one key's value
    assert "1 of %d keys differ" % k.size in se.first_key_difference(c, k, e.keys, e.xs, e.ys)
    assert "shape" in se.first_key_difference(c, k[:, 1:], e.keys, e.xs, e.ys)
    want = se.sorted_expected(e)
    assert want.size == np.count_nonzero(e.keys) and np.all(want[:-1] > want[1:])
    feats = e.feats.copy()
    assert se.feats_difference(feats, e.feats) is None
    feats["x"][3] += 1
    assert "feature 3" in se.feats_difference(feats, e.feats)
