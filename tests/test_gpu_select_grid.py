"""Selection grid (klt_set_select_grid, tc.selectionGrid) on the GPU: every record equals the list composed from the pinned oracle's pieces
(tests/select_grid_expected.py) exactly -- x, y and val -- through the filter in front of the rank placement, the greedy walk under a
quota, the placement behind the sort, the candidate prefilter and its repeat, and the Python API."""
import numpy as np
import pytest

from helpers import _api_modules, make_tc, params_from_tc
from select_grid_expected import (N_DRAWS, accepted_sequence, apply_quota, grid_case, grid_dims, live_counts, select_grid_expected)
from select_mask_expected import (KLT_NOT_FOUND, REPLACING_SOME, SELECTING_ALL, drop_every_third, frame, rect_mask, same_records,
                                  select_expected)

pytestmark = pytest.mark.gpu
KLT_OPT_SELECT_AFFINE_STATE, KLT_OPT_TOPK_PREFILTER, KLT_OPT_SELECT_PARALLEL_NMS = 4, 5, 8
PATH_FILTER, PATH_WALK = 1, 2
RANK_LIMIT, PREFILTER_FROM = 98304, 262144

_frames, _A, _plain = {}, {}, {}


def frame_of(ncols, nrows):
    if (ncols, nrows) not in _frames:
        _frames[ncols, nrows] = frame(ncols, nrows)
    return _frames[ncols, nrows]


def plain(ncols, nrows, n, **tc_attrs):
    """the selection without a grid, and the list a replacement starts from (every third feature lost); never modified"""
    key = (ncols, nrows, n, tuple(sorted(tc_attrs.items())))
    if key not in _plain:
        sel = select_expected(params_from_tc(make_tc(**tc_attrs)), frame_of(ncols, nrows).astype(np.float32), n)
        start = drop_every_third(sel)
        sel.setflags(write=False)
        start.setflags(write=False)
        _plain[key] = (sel, start)
    return _plain[key]


def members(ncols, nrows, mode=SELECTING_ALL, n=None, mask=None, **tc_attrs):
    """A of a frame (for a replacement: from plain(..., n)'s start list), computed once per case and never modified"""
    key = (ncols, nrows, mode, n if mode == REPLACING_SOME else None, mask, tuple(sorted(tc_attrs.items())))
    if key not in _A:
        start = plain(ncols, nrows, n, **tc_attrs)[1] if mode == REPLACING_SOME else None
        m = rect_mask(ncols, nrows) if mask == "rect" else None
        _A[key] = accepted_sequence(params_from_tc(make_tc(**tc_attrs)), frame_of(ncols, nrows).astype(np.float32), mode, start, m)
        _A[key].setflags(write=False)
    return _A[key]


def expected(ncols, nrows, n, grid, mode=SELECTING_ALL, mask=None, **tc_attrs):
    """(list the selection starts from, expected records)"""
    start = plain(ncols, nrows, n, **tc_attrs)[1] if mode == REPLACING_SOME else None
    m = rect_mask(ncols, nrows) if mask == "rect" else None
    want = select_grid_expected(params_from_tc(make_tc(**tc_attrs)), frame_of(ncols, nrows).astype(np.float32), n, grid, mode, start, m,
                                members(ncols, nrows, mode, n, mask, **tc_attrs))
    return start, want


class Ctx:
    """a context with the shared frame of one size in slot 0, its pyramids built"""

    def __init__(self, ncols, nrows, options=(), **tc_attrs):
        from pyfeaturetrack_amd.backend import Context
        self.size = (ncols, nrows)
        self.c = Context(0)
        try:
            self.c.configure(make_tc(**tc_attrs))
            for opt, value in options:
                self.c.set_option(opt, value)
            self.c.upload(0, frame_of(ncols, nrows))
            self.c.build_pyramids(0, sync=True)
        except Exception:
            self.c.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.close()

    def select(self, n, mode=SELECTING_ALL, start=None, use_pyramid=True):
        return self.c.select(0, n, mode, start, use_pyramid)[0]

    def candidates(self):
        import ctypes as C
        nx, ny = C.c_int(), C.c_int()
        self.c._check(self.c._lib.klt_select_dims(self.c._h, 3, C.byref(nx), C.byref(ny)))
        return nx.value * ny.value


def check(got, want, what):
    assert np.array_equal(got["val"], want["val"]), "%s: status / value words" % (what,)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"]), "%s: positions" % (what,)


def found(fl):
    return int((fl["val"] >= 0).sum())


# ---- the three basic cases, through the parallel passes (filter + rank placement) and through the walk -----------------------------
WALK = ((KLT_OPT_SELECT_PARALLEL_NMS, 0),)


@pytest.mark.parametrize("options, path", [((), PATH_FILTER), (WALK, PATH_WALK)], ids=["passes", "walk"])
def test_320x240_list_fills_and_list_does_not_fill(options, path):
    ncols, nrows, grid = 320, 240, (64, 48, 3)
    A = members(ncols, nrows)
    taken, _ = apply_quota(A, np.full(25, 3), 50, ncols, grid)
    assert len(A) == 303 and len(taken) == 50 and taken[:30].tolist() == list(range(30)) and taken[30] != 30, \
        "303 accepted, the first member turned away is A[30]"
    with Ctx(ncols, nrows, options) as g:
        assert g.c.select_grid_path() == 0
        g.c.set_select_grid(grid)
        assert g.c.select_grid_path() == 0
        want = expected(ncols, nrows, 50, grid)[1]
        assert found(want) == 50
        check(g.select(50), want, "n = 50: the list fills")
        assert g.c.select_grid_path() == path
        want = expected(ncols, nrows, 100, grid)[1]
        assert found(want) == 75 and (want["val"][75:] == KLT_NOT_FOUND).all() and (want["x"][75:] == -1).all()
        for use_pyramid in (True, False):
            check(g.select(100, use_pyramid=use_pyramid), want, "n = 100: 75 kept, then KLT_NOT_FOUND")
        assert live_counts(want, ncols, nrows, grid).max() == 3
        assert g.c.select_grid_path() == path


@pytest.mark.parametrize("options, path", [((), PATH_FILTER), (WALK, PATH_WALK)], ids=["passes", "walk"])
def test_333x217_partial_cells_and_the_barrier_tables(options, path):
    ncols, nrows, grid = 333, 217, (50, 70, 2)
    assert ncols % 4 and ncols % grid[0] == 33 and grid_dims(ncols, nrows, grid) == (7, 4)
    want = expected(ncols, nrows, 60, grid)[1]
    assert found(want) == 40
    last_column = want[(want["val"] >= 0) & (want["x"] >= 300)]
    assert len(last_column), "no feature in the narrow last column of cells: the case shows nothing"
    with Ctx(ncols, nrows, options) as g:
        g.c.set_select_grid(grid)
        check(g.select(60), want, "333 x 217")
        assert g.c.select_score_path()[0] == 0, "the barrier-coupled table kernels were expected at a width that is no multiple of 4"
        assert g.c.select_grid_path() == path


@pytest.mark.parametrize("options, path", [((), PATH_FILTER), (WALK, PATH_WALK)], ids=["passes", "walk"])
def test_replacement_and_affine_state(options, path):
    ncols, nrows, n, grid = 320, 240, 100, (64, 48, 3)
    start, want = expected(ncols, nrows, n, grid, REPLACING_SOME)
    lost = start["val"] < 0
    filled = lost & (want["val"] >= 0)
    assert lost.sum() == 34 and (live_counts(start, ncols, nrows, grid) >= 3).sum() == 12 and filled.sum() == 25
    with Ctx(ncols, nrows, options, affineConsistencyCheck=2) as g:
        g.c.set_select_grid(grid)
        got = g.select(n, REPLACING_SOME, start)
        check(got, want, "replacement")
        assert got[~lost].tobytes() == np.array(start)[~lost].tobytes(), "live records are untouched"
        assert g.c.select_grid_path() == path
        # an affine state selected: exactly the filled slots start over.  The state of every feature is made valid first, by an affine
        # tracking step of the full list from the frame into itself
        g.c.upload(1, frame_of(ncols, nrows))
        g.c.build_pyramids(1, sync=True)
        g.c.affine_alloc(0, n)
        g.c.track_affine(0, 1, plain(ncols, nrows, n)[0], 0)
        before = g.c.affine_download(0, n)
        assert before["valid"][filled].any() and before["valid"][lost & ~filled].any() and before["valid"][~lost].any()
        g.c.set_option(KLT_OPT_SELECT_AFFINE_STATE, 0)
        try:
            got = g.select(n, REPLACING_SOME, start)
        finally:
            g.c.set_option(KLT_OPT_SELECT_AFFINE_STATE, -1)
        check(got, want, "replacement with an affine state")
        after = g.c.affine_download(0, n)
        assert not after["valid"][filled].any() and (after["aff_x"][filled] == -1).all() and (after["Axx"][filled] == 1).all()
        assert after[~filled].tobytes() == before[~filled].tobytes(), "a slot that was not filled lost its affine state"


# ---- placement behind the sort: more accepted candidates than the ranking takes ------------------------------------------------------
@pytest.mark.parametrize("mindist", [1, 0])
def test_480x360_placement_after_the_sort(mindist):
    ncols, nrows, grid = 480, 360, (96, 90, 5)
    with Ctx(ncols, nrows, mindist=mindist) as g:
        g.c.set_select_grid(grid)
        for n, fills in ((60, True), (200, False)):                  # 20 cells of 5: at most 100 are kept
            for mode in (SELECTING_ALL, REPLACING_SOME):
                start, want = expected(ncols, nrows, n, grid, mode, mindist=mindist)
                free = np.ones(n, bool) if start is None else start["val"] < 0
                assert bool((want["val"][free] >= 0).all()) == fills
                check(g.select(n, mode, start), want, (mindist, n, mode))
        assert g.candidates() == 126000 > RANK_LIMIT
        assert g.c.select_grid_path() == PATH_WALK


# ---- the candidate prefilter and its repeat ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefilter", [1, 0])
def test_768x512_prefilter_and_repeat(prefilter):
    ncols, nrows, n = 768, 512, 20
    tight, wide = (256, 256, 2), (256, 256, 50)
    with Ctx(ncols, nrows, ((KLT_OPT_TOPK_PREFILTER, prefilter),)) as g:
        g.select(n)                                                  # (allocations, and the number of passes a selection here needs)
        assert g.candidates() == 320016 > PREFILTER_FROM
        def two_halves(mode, start, want, what):
            """the selection in its two halves, twice: the second time the number of passes enqueued ahead is what the first one needed,
            so klt_select_finish reports a rewritten list only for the repeat with every candidate"""
            for _ in range(2):
                g.c.featbuf_upload(7, want if start is None else start)
                g.c.select_begin(0, mode, True, 7, n)
                repeated = g.c.select_finish()
                check(g.c.featbuf_download(7, n), want, what)
            return repeated
        for mode in (SELECTING_ALL, REPLACING_SOME):
            start, want = expected(ncols, nrows, n, tight, mode)
            free = np.ones(n, bool) if start is None else start["val"] < 0
            assert found(want[free]) <= 12 and (want["val"][free] < 0).any(), "the kept members must run out"
            g.c.set_select_grid(tight)
            repeated = two_halves(mode, start, want, ("q = 2", mode))
            assert repeated == bool(prefilter), "the cut's candidates run out: the repeat with every candidate (and only behind a cut)"
            assert g.c.select_grid_path() == PATH_FILTER
            start, want = expected(ncols, nrows, n, wide, mode)
            assert (want["val"] >= 0).all()
            g.c.set_select_grid(wide)
            assert not two_halves(mode, start, want, ("q = 50", mode)), "q = 50 holds without a repeat"
        # a replacement on prepared scores
        for grid in (tight, wide):
            start, want = expected(ncols, nrows, n, grid, REPLACING_SOME)
            g.c.set_select_grid(grid)
            g.c.select_prepare(0)
            check(g.select(n, REPLACING_SOME, start), want, ("prepared scores", grid))
            if prefilter:
                from pyfeaturetrack_amd.backend import KltBackendError
                with pytest.raises(KltBackendError, match="prepared scores"):
                    g.c.select_intermediate(3)                       # the prepared scores WERE used


def test_768x512_walk_behind_the_prefilter():
    ncols, nrows, n, grid = 768, 512, 20, (256, 256, 2)
    with Ctx(ncols, nrows, WALK) as g:
        g.c.set_select_grid(grid)
        for mode in (SELECTING_ALL, REPLACING_SOME):
            start, want = expected(ncols, nrows, n, grid, mode)
            check(g.select(n, mode, start), want, mode)
        assert g.c.select_grid_path() == PATH_WALK


def test_512x260_quota_walk_with_the_cell_grid_in_global_memory():
    """mindist 2: a cell grid of 256 x 130 words = 133 120 bytes, just past the 131 072 the walk keeps in LDS -- the walk under a quota with
    its cell grid in global memory, and before a grid is set the plain walk on the same frame"""
    ncols, nrows, grid, mindist = 512, 260, (64, 52, 40), 2
    assert grid_dims(ncols, nrows, grid) == (8, 5) and (ncols // mindist) * (nrows // mindist) * 4 == 133120 > 131072
    assert len(members(ncols, nrows, mindist=mindist)) == 19491
    does_not_fill = expected(ncols, nrows, 2000, grid, mindist=mindist)[1]
    assert found(does_not_fill) == 1600 and live_counts(does_not_fill, ncols, nrows, grid).max() == 40, "every cell at its cap of 40"
    fills = expected(ncols, nrows, 1000, grid, mindist=mindist)[1]
    assert found(fills) == 1000
    start, replaced = expected(ncols, nrows, 2000, grid, REPLACING_SOME, mindist=mindist)
    assert (start["val"] < 0).sum() == 667 and (replaced["val"] < 0).sum() == 130
    with Ctx(ncols, nrows, WALK, mindist=mindist) as g:
        check(g.select(2000), plain(ncols, nrows, 2000, mindist=mindist)[0], "no grid: the plain walk")
        pick = g.c.select_pick_path()
        assert pick["walk"] == 0 and pick["grid"] == 1 and g.candidates() < PREFILTER_FROM
        g.c.set_select_grid(grid)
        for n, mode, first, want in ((2000, SELECTING_ALL, None, does_not_fill), (1000, SELECTING_ALL, None, fills),
                                     (2000, REPLACING_SOME, start, replaced)):
            check(g.select(n, mode, first), want, (n, mode))
            assert g.c.select_grid_path() == PATH_WALK and g.c.select_pick_path()["grid"] == 1


# ---- composition and state -----------------------------------------------------------------------------------------------------------
def test_mask_and_grid_compose():
    ncols, nrows, n, grid = 320, 240, 100, (64, 48, 3)
    with Ctx(ncols, nrows) as g:
        g.c.set_select_mask(rect_mask(ncols, nrows))
        g.c.set_select_grid(grid)
        for mode in (SELECTING_ALL, REPLACING_SOME):
            start, want = expected(ncols, nrows, n, grid, mode, mask="rect")
            assert not same_records(want, expected(ncols, nrows, n, grid, mode)[1])
            check(g.select(n, mode, start), want, ("mask + grid", mode))


def test_grid_set_removed_and_set_again_and_one_cell():
    ncols, nrows, n, grid = 320, 240, 100, (64, 48, 3)
    sel, start = plain(ncols, nrows, n)
    rep = select_expected(params_from_tc(make_tc()), frame_of(ncols, nrows).astype(np.float32), n, REPLACING_SOME, start)
    want = expected(ncols, nrows, n, grid)[1]
    assert not same_records(want, sel)
    with Ctx(ncols, nrows) as g:
        for _ in range(2):
            g.c.set_select_grid(grid)
            check(g.select(n), want, "grid set")
            g.c.set_select_grid(None)
            check(g.select(n), sel, "grid removed")
            check(g.select(n, REPLACING_SOME, start), rep, "grid removed, replacement")
        g.c.set_select_grid((0, -5, 123456))                         # cell_width == 0: no grid, whatever else the struct holds
        check(g.select(n), sel, "cell_width 0")
        # one cell with room for every slot: the plain selection bit for bit
        for one in ((ncols, nrows, n), (ncols + 1000, 70000, 65535), (2 ** 31 - 1, 2 ** 31 - 1, n)):
            g.c.set_select_grid(one)
            assert g.select(n).tobytes() == g.select(n).tobytes()
            got = g.select(n)
            assert np.array_equal(got["x"], sel["x"]) and np.array_equal(got["y"], sel["y"]) and np.array_equal(got["val"], sel["val"])
            check(g.select(n, REPLACING_SOME, start), rep, ("one cell, replacement", one))
        g.c.set_select_grid((ncols, nrows, 37))                      # one cell of 37: the first 37, then KLT_NOT_FOUND
        got = g.select(n)
        assert same_records(got[:37], sel[:37]) and (got["val"][37:] == KLT_NOT_FOUND).all()


def test_errors_and_a_grid_set_while_a_selection_is_pending():
    from pyfeaturetrack_amd.backend import KltBackendError
    ncols, nrows, n, grid = 320, 240, 100, (64, 48, 3)
    want = expected(ncols, nrows, n, grid)[1]
    with Ctx(ncols, nrows) as g:
        g.c.set_select_grid(grid)
        for bad in ((-1, 48, 3), (64, 0, 3), (64, -48, 3), (64, 48, 0), (64, 48, 65536), (64, 48, -1)):
            with pytest.raises(KltBackendError, match="error -1"):
                g.c.set_select_grid(bad)
        check(g.select(n), want, "after the refused calls: the grid stays")
        g.c.select_begin(0, SELECTING_ALL, True, 7, n)
        for call in (lambda: g.c.set_select_grid((32, 32, 1)), lambda: g.c.set_select_grid(None)):
            with pytest.raises(KltBackendError, match="error -3.*pending"):
                call()
        g.c.select_finish()
        check(g.c.featbuf_download(7, n), want, "the pending selection kept its grid")
        check(g.select(n), want, "the context selects on")


@pytest.mark.parametrize("mode", [SELECTING_ALL, REPLACING_SOME], ids=["all", "replace"])
def test_no_additional_launch_without_a_grid(mode):
    ncols, nrows, n, grid = 333, 217, 100, (50, 70, 2)
    start = plain(ncols, nrows, n)[1] if mode == REPLACING_SOME else None

    def launches(g):
        g.c.timing_enable(1)                                     # (resets the figures)
        g.select(n, mode, start)
        counts = {t["name"]: t["launches"] for t in g.c.timing_read() if t["launches"]}
        g.c.timing_enable(0)
        return counts
    with Ctx(ncols, nrows) as g:                                 # a context that never had a grid
        g.select(n, mode, start)
        g.select(n, mode, start)
        g.select(n, mode, start)
        never = launches(g)
    with Ctx(ncols, nrows) as g:
        g.select(n, mode, start)
        g.c.set_select_grid(grid)
        g.select(n, mode, start)
        with_grid = launches(g)
        g.c.set_select_grid(None)
        g.select(n, mode, start)
        after = launches(g)
    assert after == never, (never, after)
    assert sum(with_grid.values()) >= sum(never.values())


# ---- seeded draws --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_context():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("k", range(N_DRAWS))
def test_seeded_draw(shared_context, k):
    ctx, c = shared_context, grid_case(k)
    t = c["t"]
    ctx.set_select_grid(None)
    ctx.set_select_mask(None)
    ctx.configure(c["tc"])
    ctx.upload(0, c["frame"])
    if c["mask"] is not None:
        ctx.set_select_mask(np.ascontiguousarray(c["mask"]))
    ctx.set_select_grid(c["grid"])
    try:
        for option in (None, KLT_OPT_SELECT_PARALLEL_NMS):
            if option is not None:
                ctx.set_option(option, 0)
            try:
                got = ctx.select(0, t["n"], t["mode"], c["start"], False)[0]
            finally:
                if option is not None:
                    ctx.set_option(option, 1)
            check(got, c["want"], (t, "walk" if option else "default"))
    finally:
        ctx.set_select_grid(None)
        ctx.set_select_mask(None)


# ---- Python API ----------------------------------------------------------------------------------------------------------------------
def _recs(fl):
    out = np.zeros(len(fl), [("x", np.float32), ("y", np.float32), ("val", np.int32)])
    out["x"], out["y"], out["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return out


def test_python_api_select_and_replace_under_a_grid():
    sgf, _ = _api_modules()
    ncols, nrows, n, grid = 320, 240, 100, (64, 48, 3)
    img = frame_of(ncols, nrows)
    sel = plain(ncols, nrows, n)[0]
    tc = make_tc(selectionGrid=grid)
    check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), expected(ncols, nrows, n, grid)[1], "KLTSelectGoodFeatures")
    tc.selectionGrid = list(grid)
    fl = sgf.KLTSelectGoodFeatures(tc, img, n)
    start, want = expected(ncols, nrows, n, grid, REPLACING_SOME)
    for i, f in enumerate(fl):                                   # the list the expected replacement starts from
        f.x, f.y, f.val = int(start["x"][i]), int(start["y"][i]), int(start["val"][i])
    sgf.KLTReplaceLostFeatures(tc, img, fl)
    check(_recs(fl), want, "KLTReplaceLostFeatures")
    tc.selectionGrid = None
    check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), sel, "grid cleared")
    tc.selectionGrid = grid
    sgf.KLTSelectGoodFeatures(tc, img, n)
    check(_recs(sgf.KLTSelectGoodFeatures(make_tc(), img, n)), sel, "a tracking context without a grid after one with")
    for bad, error in (((64, 48), TypeError), ((64, 48, 0), ValueError), ("grid", TypeError)):
        tc.selectionGrid = bad
        with pytest.raises(error):
            sgf.KLTSelectGoodFeatures(tc, img, n)


def test_track_sequence_under_a_grid_equals_the_host_loop():
    from pyfeaturetrack_amd import storeFeatures as sf, synth
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    sgf, tf = _api_modules()
    ncols, nrows, n, nf, grid = 320, 240, 100, 4, (64, 48, 3)
    base = synth.synth_base(ncols, nrows, 17)
    frames = [synth.synth_frame(ncols, nrows, 17, k, shift=(1.3, -0.8), base=base) for k in range(nf)]
    frames[2] = frames[2].copy()
    frames[2][nrows // 8:nrows // 2, ncols // 8:ncols // 2] = 100            # features are lost here and replaced

    def make(**kw):
        return make_tc(levels=2, ss=4, max_residue=10.0, sequentialMode=True, **kw)
    tc = make(selectionGrid=grid)
    want = sf.KLTCreateFeatureTable(nf, n)
    fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
    sf.KLTStoreFeatureList(fl, want, 0)
    assert 0 < found(_recs(fl)) < n and live_counts(_recs(fl), ncols, nrows, grid).max() == 3
    replaced = 0
    for k in range(1, nf):
        tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
        lost = np.array([f.val < 0 for f in fl])
        sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
        replaced += int((_recs(fl)["val"][lost] >= 0).sum())
        sf.KLTStoreFeatureList(fl, want, k)
    assert replaced > 0, "nothing was replaced: the clip shows nothing"
    for kw in ({}, {"prefetch": False}):
        got = KLTTrackSequence(make(selectionGrid=grid), iter(frames), n, **kw)
        assert np.array_equal(got.val, want.val) and np.array_equal(got.x, want.x) and np.array_equal(got.y, want.y), kw
    plain_table = KLTTrackSequence(make(), iter(frames), n)
    assert not np.array_equal(plain_table.x, want.x), "the grid changes nothing on this clip"
    tc = make(selectionGrid=(64, 48))
    with pytest.raises(TypeError):
        KLTTrackSequence(tc, iter(frames), n)
