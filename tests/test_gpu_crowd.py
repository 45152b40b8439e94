"""The crowding check (klt_crowd_check*) on the device against the plain restatement of the rule
(tests/crowd_expected.py), on every byte of `out` and of the crowd records.  There is no tolerance: a difference is a bug in the kernels
or in the restatement's transcription of the rule."""
import numpy as np
import pytest

from crowd_expected import (CROWD_DTYPE, KLT_CROWDED, border_pairs, chain, crowd_check_expected, crowd_records, live_pairs_within,
                            non_candidate_kinds, random_list, records)

pytestmark = pytest.mark.gpu

FB_OUT, FB_PREV, FB_CROWD = 100, 101, 102
NCOLS, NROWS = 320, 240


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_same(got_out, got_crowd, want_out, want_crowd, what):
    """bytes: the lists hold NaN coordinates, and -0 is not +0"""
    for name, got, want in (("out", got_out, want_out), ("crowd", np.asarray(got_crowd).view(CROWD_DTYPE), want_crowd)):
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1))
            raise AssertionError("%s: %d of %d %s records differ, first at %d: got %r, want %r" % (what, bad.size, len(got), name, bad[0],
                                                                                                   got[bad[0]], want[bad[0]]))


def mixed_list(n, seed):
    """random records with ages 0 .. 4; from 600 records on with every kind of non-candidate mixed in"""
    out, prev = random_list(n, NCOLS, NROWS, seed)
    if n >= 600:
        non, edge = non_candidate_kinds(out, NCOLS, NROWS, start=1, step=max(1, n // 37))
        assert len(non) >= 20 and len(edge) == 4
    return out, prev


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 600, 8193])
def test_kernels_equal_the_rule_across_counts_and_distances(ctx, n):
    """n across one wavefront, one pass of the resolve workgroup's 1024 lanes and several; d = 1 (r = 0: the same pixel only), 2, 10 (dense:
    most records are crowded) and 33 (r = 32, wider than the minimum cell of 16 pixels)"""
    out, prev = mixed_list(n, seed=40 + n)
    for d in (1, 2, 10, 33):
        ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=d)
        want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, d)
        got_out, got_crowd, flagged = ctx.crowd_check(out, prev)
        assert_same(got_out, got_crowd, want_out, want_crowd, "n %d, d %d" % (n, d))
        assert flagged == int((want_crowd["val"] == 2).sum())
        assert ctx.crowd_check_path() == 1
        if n < 600:                                          # (the mixed lists hold val > 0 records: live, but no candidates)
            assert live_pairs_within(got_out, d - 1, NCOLS, NROWS) == 0
        print("n %d, d %d: %d kept, %d crowded, %d rounds" % (n, d, (want_crowd["val"] == 1).sum(), flagged, ctx.crowd_check_rounds()))
    if n >= 600:
        assert flagged > n // 2                              # d = 33 on this frame: most records are crowded
    want_out, want_crowd = crowd_check_expected(out, None, NCOLS, NROWS, 10)         # without prev: list order decides
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    got_out, got_crowd, _ = ctx.crowd_check(out, None)
    assert_same(got_out, got_crowd, want_out, want_crowd, "n %d without prev" % n)


@pytest.mark.parametrize("n", [24576, 24577])
def test_lists_at_the_lds_threshold(ctx, n):
    """the resolve kernel keeps pixel and state of up to 24 576 candidates in LDS; one record more and both live in the context's scratch"""
    out, prev = random_list(n, NCOLS, NROWS, seed=5)
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=3)
    want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 3)
    got_out, got_crowd, flagged = ctx.crowd_check(out, prev)
    assert_same(got_out, got_crowd, want_out, want_crowd, "%d records" % n)
    assert 1000 < flagged < n - 1000


@pytest.mark.parametrize("name,kw", [("along x", dict()), ("along x, ages rising", dict(reverse=True)),
                                     ("diagonal", dict(dx=1, dy=1, x0=2.0, y0=2.0))], ids=["x", "x-reversed", "diagonal"])
def test_chains_take_as_many_rounds_as_they_are_long(ctx, name, kw):
    """300 candidates spaced r apart with ages falling along the line: each waits for its older neighbour, so the rounds are 300 -- the
    loop ends on its condition.  The diagonal chain (r = 7 on cells of 16 pixels) crosses a cell border in x and in y every other step."""
    r = 7 if "diagonal" in name else 9
    ncols, nrows = (2400, 2400) if "diagonal" in name else (3000, 64)
    out, prev = chain(300, r, **kw)
    ctx.set_crowd_params(ncols=ncols, nrows=nrows, min_distance=r + 1)
    want_out, want_crowd = crowd_check_expected(out, prev, ncols, nrows, r + 1)
    got_out, got_crowd, flagged = ctx.crowd_check(out, prev)
    assert_same(got_out, got_crowd, want_out, want_crowd, name)
    order = want_crowd["val"].tolist() if not kw.get("reverse") else want_crowd["val"].tolist()[::-1]
    assert order == [1, 2] * 150 and flagged == 150
    rounds = ctx.crowd_check_rounds()
    print("chain %s: %d rounds" % (name, rounds))
    assert 1 <= rounds <= 300


def test_negative_and_saturating_ages(ctx):
    """a negative age in prev counts as 0 (index then decides), INT32_MAX - 1 and INT32_MAX both come back as INT32_MAX; identical
    positions keep the lowest index among equal ages, the oldest whatever its index"""
    big = 0x7FFFFFFF
    out = records([10, 12, 100, 200, 50.2, 50.9, 50.5], [10, 10, 10, 10, 60.1, 60.7, 60.0])
    for ages, d in (([-5, 0, big, big - 1, 3, 3, 3], 10), ([-5, 0, big, big - 1, 0, 1, 5], 1), ([-1, -big - 1, 0, 0, -7, -7, -8], 1)):
        prev = crowd_records(ages)
        ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=d)
        want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, d)
        got_out, got_crowd, _ = ctx.crowd_check(out, prev)
        assert_same(got_out, got_crowd, want_out, want_crowd, "ages %r" % (ages,))
    assert want_crowd["val"].tolist() == [1, 1, 1, 1, 1, 2, 2] and want_crowd["winner"].tolist()[5:] == [4, 4]
    _, c = crowd_check_expected(out, crowd_records([-5, 0, big, big - 1, 0, 1, 5]), NCOLS, NROWS, 10)
    assert c["age"].tolist() == [1, 0, big, big, 0, 0, 6] and c["winner"].tolist() == [-1, 0, -1, -1, 6, 6, -1]


def test_cell_borders_and_frame_corners(ctx):
    """pairs exactly r and r + 1 apart across a cell border, in x, in y and diagonally; candidates at (0, 0) and (ncols - 1, nrows - 1)"""
    out, _ = border_pairs(NCOLS, NROWS, 9, 16)
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    want_out, want_crowd = crowd_check_expected(out, None, NCOLS, NROWS, 10)
    assert want_crowd["val"].tolist() == [1, 2] * 3 + [1, 1] * 3 + [1, 1]
    got_out, got_crowd, flagged = ctx.crowd_check(out, None)
    assert_same(got_out, got_crowd, want_out, want_crowd, "border pairs")
    assert flagged == 3
    # a frame that is no multiple of the cell: the last cell column and row are short; both corners again
    out = records([0.0, 8.9, 300.0, 308.99, 150.0], [0.0, 0.5, 228.0, 236.99, 100.0])
    ctx.set_crowd_params(ncols=309, nrows=237, min_distance=10)
    want_out, want_crowd = crowd_check_expected(out, None, 309, 237, 10)
    assert want_crowd["val"].tolist() == [1, 2, 1, 2, 1]
    got_out, got_crowd, _ = ctx.crowd_check(out, None)
    assert_same(got_out, got_crowd, want_out, want_crowd, "309 x 237")


def test_the_grid_at_its_largest(ctx):
    """3840 x 2160, 20 000 records, d = 10: 240 x 135 cells"""
    out, prev = random_list(20000, 3840, 2160, seed=8)
    ctx.set_crowd_params(ncols=3840, nrows=2160, min_distance=10)
    want_out, want_crowd = crowd_check_expected(out, prev, 3840, 2160, 10)
    got_out, got_crowd, flagged = ctx.crowd_check(out, prev)
    assert_same(got_out, got_crowd, want_out, want_crowd, "4K")
    print("4K: %d crowded of 20000, %d rounds" % (flagged, ctx.crowd_check_rounds()))
    assert flagged > 500 and live_pairs_within(got_out[:4000], 9, 3840, 2160) == 0


def test_a_batch_of_three_lists_equals_three_single_calls(ctx):
    n = 300
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    lists = []
    for i in range(3):
        out, prev = random_list(n, NCOLS, NROWS, seed=70 + i)
        out["val"][i * 40:i * 90] = -3                       # another number of candidates in every list
        lists.append((out, prev if i != 1 else None))        # the second one without a previous step
    triples = []
    for i, (out, prev) in enumerate(lists):
        ctx.featbuf_upload(200 + 3 * i, out)
        if prev is not None:
            ctx.featbuf_upload(201 + 3 * i, prev.view(out.dtype))
        triples.append((200 + 3 * i, 201 + 3 * i if prev is not None else -1, 202 + 3 * i))
    ctx.crowd_check_batch_async(triples, n)
    assert ctx.crowd_check_path() == 2
    for i, (out, prev) in enumerate(lists):
        want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 10)
        assert (want_crowd["val"] == 2).sum() > 20
        assert_same(ctx.featbuf_download(triples[i][0], n), ctx.crowd_download(triples[i][2], n), want_out, want_crowd, "list %d of the batch" % i)
        single_out, single_crowd, _ = ctx.crowd_check(out, prev)
        assert ctx.crowd_check_path() == 1
        assert_same(single_out, single_crowd, want_out, want_crowd, "list %d alone" % i)
    from pyfeaturetrack_amd.backend import KltBackendError
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.crowd_check_batch_async([triples[0], (triples[1][0], -1, triples[0][0])], n)      # crowd records into another list
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.crowd_check_batch_async([triples[0], (triples[1][0], -1, triples[0][2])], n)      # two lists share fb_crowd
    with pytest.raises(KltBackendError, match="share fb_out"):
        ctx.crowd_check_batch_async([triples[0], (triples[0][0], -1, triples[1][2])], n)      # two entries rewrite one list
    with pytest.raises(KltBackendError, match="bad argument"):
        ctx.crowd_check_batch_async([triples[0]], -1)
    out, prev = lists[2]                                     # ... and the context works on
    ctx.featbuf_upload(triples[2][0], out)
    ctx.crowd_check_batch_async([triples[2]], n)
    want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 10)
    assert_same(ctx.featbuf_download(triples[2][0], n), ctx.crowd_download(triples[2][2], n), want_out, want_crowd, "after the refused batches")


def test_resident_lists_with_and_without_prev(ctx):
    out, prev = mixed_list(600, seed=12)
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    for fb_prev, p in ((FB_PREV, prev), (-1, None)):
        want_out, want_crowd = crowd_check_expected(out, p, NCOLS, NROWS, 10)
        ctx.featbuf_upload(FB_OUT, out)
        ctx.featbuf_upload(FB_PREV, prev.view(out.dtype))
        ctx.crowd_check_async(FB_OUT, fb_prev, FB_CROWD, len(out))
        assert_same(ctx.featbuf_download(FB_OUT, len(out)), ctx.crowd_download(FB_CROWD, len(out)), want_out, want_crowd, "prev %d" % fb_prev)
        assert ctx.featbuf_download(FB_PREV, len(out)).tobytes() == prev.tobytes()
    # n == 0: KLT_OK and nothing is written
    before_out, before_crowd = ctx.featbuf_download(FB_OUT, 20), ctx.featbuf_download(FB_CROWD, 20)
    ctx.crowd_check_async(FB_OUT, FB_PREV, FB_CROWD, 0)
    ctx.crowd_check_batch_async([(FB_OUT, FB_PREV, FB_CROWD)], 0)
    ctx.sync()
    assert ctx.featbuf_download(FB_OUT, 20).tobytes() == before_out.tobytes() and ctx.featbuf_download(FB_CROWD, 20).tobytes() == before_crowd.tobytes()
    got_out, got_crowd, flagged = ctx.crowd_check(out[:0], None)
    assert len(got_out) == 0 and len(got_crowd) == 0 and flagged == 0


def test_a_second_call_gives_the_same_bytes(ctx):
    """the same lists uploaded again: the same bytes (nothing of a call survives in the scratch); the check on what it left, with the
    ages it left: nothing further is flagged and every kept record is a step older"""
    out, prev = mixed_list(600, seed=77)
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 10)
    got = []
    for _ in range(2):
        ctx.featbuf_upload(FB_OUT, out)
        ctx.featbuf_upload(FB_PREV, prev.view(out.dtype))
        ctx.crowd_check_async(FB_OUT, FB_PREV, FB_CROWD, len(out))
        got.append((ctx.featbuf_download(FB_OUT, len(out)), ctx.crowd_download(FB_CROWD, len(out))))
        assert_same(got[-1][0], got[-1][1], want_out, want_crowd, "call %d" % len(got))
    again_out, again_crowd = crowd_check_expected(want_out, want_crowd, NCOLS, NROWS, 10)
    assert not (again_crowd["val"] == 2).any()
    ctx.crowd_check_async(FB_OUT, FB_CROWD, FB_PREV, len(out))            # the buffers change roles: this step's records are the next one's prev
    assert_same(ctx.featbuf_download(FB_OUT, len(out)), ctx.crowd_download(FB_PREV, len(out)), again_out, again_crowd, "the check on its own result")


def test_error_returns_leave_the_context_working(ctx):
    from pyfeaturetrack_amd.backend import KltBackendError
    n = 64
    FB_OUT, FB_PREV, FB_CROWD, FB_VIEW = 110, 111, 112, 113      # buffers of this test's own: exactly n records each
    out, prev = random_list(n, NCOLS, NROWS, seed=5)
    ctx.featbuf_upload(FB_OUT, out)
    ctx.featbuf_upload(FB_PREV, prev.view(out.dtype))
    ctx.featbuf_view(FB_VIEW, FB_OUT, 0, n)
    ctx.set_crowd_params(mode=0)
    for call in (lambda: ctx.crowd_check_async(FB_OUT, FB_PREV, FB_CROWD, n), lambda: ctx.crowd_check(out, prev),
                 lambda: ctx.crowd_check_batch_async([(FB_OUT, FB_PREV, FB_CROWD)], n)):
        with pytest.raises(KltBackendError, match="crowding check is off"):
            call()
    for bad in (dict(mode=2), dict(mode=-1), dict(min_distance=0), dict(min_distance=-4), dict(ncols=0), dict(nrows=65536), dict(ncols=-1)):
        with pytest.raises(KltBackendError, match="crowding"):
            ctx.set_crowd_params(**dict(dict(ncols=NCOLS, nrows=NROWS, min_distance=10), **bad))
    ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=10)
    for args, pattern in (((FB_OUT, FB_PREV, FB_OUT, n), "distinct"), ((FB_OUT, FB_PREV, FB_PREV, n), "distinct"),
                          ((FB_OUT, FB_PREV, FB_VIEW, n), "distinct"),                    # a view of fb_out: the same address under another index
                          ((FB_OUT, FB_PREV, -1, n), "feature buffer"), ((FB_OUT, -2, FB_CROWD, n), "fb_prev"),
                          ((FB_OUT, FB_PREV, FB_CROWD, n + 1), "not set"), ((999, FB_PREV, FB_CROWD, n), "not set"),
                          ((FB_OUT, 998, FB_CROWD, n), "not set"), ((FB_OUT, FB_PREV, FB_CROWD, -1), "negative")):
        with pytest.raises(KltBackendError, match=pattern):
            ctx.crowd_check_async(*args)
        ctx.sync()
        assert ctx.featbuf_download(FB_OUT, n).tobytes() == out.tobytes() and ctx.featbuf_download(FB_PREV, n).tobytes() == prev.tobytes()
    want_out, want_crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 10)
    ctx.crowd_check_async(FB_OUT, FB_PREV, FB_CROWD, n)
    assert_same(ctx.featbuf_download(FB_OUT, n), ctx.crowd_download(FB_CROWD, n), want_out, want_crowd, "after the refused calls")
