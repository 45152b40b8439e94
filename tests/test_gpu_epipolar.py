"""The epipolar check (klt_epipolar_check*) on the device against the numpy restatement of the rule
(tests/epipolar_expected.py), bit for bit on every byte of `out` and of the model record.  A difference is a bug in the kernels or in the
restatement's transcription of the rule, not a tolerance."""
import numpy as np
import pytest

from epipolar_expected import (EPIPOLAR_DTYPE, KLT_EPIPOLAR_OUTLIER, epipolar_check_expected, epipolar_matrix, inside_mover, layered_clip,
                               parallax_lists, parallax_n, translation_lists)
from helpers import make_tc
from model_expected import FEAT_DTYPE, KLT_TRACKED, candidate_mask, non_candidate_kinds, records

pytestmark = pytest.mark.gpu

FB_IN, FB_OUT, FB_M = 100, 101, 102
NCOLS, NROWS = 320, 240


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_same(got_out, got_model, want_out, want_model, what):
    """bytes: the lists hold NaN coordinates, and -0 is not +0"""
    got_model, want_model = np.asarray(got_model, EPIPOLAR_DTYPE).reshape(1), np.asarray(want_model, EPIPOLAR_DTYPE).reshape(1)
    assert got_model.tobytes() == want_model.tobytes(), "%s: model record differs: got %r, want %r" % (what, got_model[0], want_model[0])
    if got_out.tobytes() != want_out.tobytes():
        bad = np.flatnonzero((got_out.view(np.uint32).reshape(-1, 4) != want_out.view(np.uint32).reshape(-1, 4)).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, first at %d: got %r, want %r" % (what, bad.size, len(got_out), bad[0],
                                                                                            got_out[bad[0]], want_out[bad[0]]))


def mixed_lists(n, seed):
    """the parallax lists on the small frame; from 600 records on with every kind of non-candidate mixed in"""
    fin, fout, _ = parallax_n(n, NCOLS, NROWS, seed)
    if n >= 600:
        non_candidate_kinds(fin, fout, NCOLS, NROWS, start=1, step=max(1, n // 37))
    return fin, fout


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 600, 8193])
def test_kernels_equal_the_rule_across_counts(ctx, n):
    """n across the eight picks, the wavefront and one tile of the gather (8192); hypotheses 1, 4 and 5 (the wavefronts of a scoring
    workgroup) and 513 (one past the decide workgroup); min_inliers 8 so that n = 8 can give a model and n = 7 none"""
    fin, fout = mixed_lists(n, seed=40 + n)
    seen = set()
    for hyp in (1, 4, 5, 513):
        kw = dict(hypotheses=hyp, seed=7 * hyp, min_inliers=8, max_error=1.0)
        ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **kw)
        want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
        got_out, got_model, flagged = ctx.epipolar_check(fin, fout)
        assert_same(got_out, got_model, want_out, want_model, "n %d, %d hypotheses" % (n, hyp))
        assert flagged == int((want_out["val"] == KLT_EPIPOLAR_OUTLIER).sum()) - int((fout["val"] == KLT_EPIPOLAR_OUTLIER).sum())
        seen.add(int(want_model["valid"]))
        assert ctx.epipolar_check_path() == 1
    print("n %d: valid outcomes %r, last model %r" % (n, sorted(seen), want_model))
    assert seen == {0} if n < 8 else 1 in seen, seen         # (eight distinct picks out of eight: one of 513 hypotheses finds them)
    if n >= 64:
        assert (want_out["val"] == KLT_EPIPOLAR_OUTLIER).any()


def test_the_parallax_scene_at_1080p(ctx):
    fin, fout, moved = parallax_lists("oblique", 11)
    ctx.set_epipolar_params(ncols=1920, nrows=1080)          # the defaults
    want_out, want_model = epipolar_check_expected(fin, fout, 1920, 1080)
    got_out, got_model, flagged = ctx.epipolar_check(fin, fout)
    assert_same(got_out, got_model, want_out, want_model, "the parallax scene")
    flag = got_out["val"] == KLT_EPIPOLAR_OUTLIER
    assert got_model["valid"] == 1 and flagged == flag.sum()
    assert (~flag & ~moved).sum() >= 0.98 * (~moved).sum() and (flag & moved).sum() >= 0.70 * moved.sum()
    from pyfeaturetrack_amd.backend import epipolar_matrix as host_matrix
    assert np.array_equal(host_matrix(got_model), epipolar_matrix(want_model).reshape(3, 3))


def test_every_outcome_and_the_asynchronous_call(ctx):
    """valid 0 (too few candidates; every hypothesis degenerate; a best score below min_inliers) and 1 through klt_epipolar_check_async
    on resident lists (valid 2, a refit that fails, takes exact integer positions: tests/test_gpu_check_draws.py, entry `valid2`);
    n = 0 enqueues nothing"""
    rs = np.random.RandomState(9)
    fin64, fout64, _ = parallax_n(64, NCOLS, NROWS, seed=5)
    tin, tout = translation_lists(64, NCOLS, NROWS, 3)
    cases = [("few", fin64[:15], fout64[:15], {}, 0),
             ("degenerate", tin, tout, {}, 0),
             ("no consensus", records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1),
              records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64)), dict(max_error=0.01, hypotheses=64), 0),
             ("refit", fin64, fout64, {}, 1)]
    for name, fin, fout, kw, valid in cases:
        kw = dict(dict(hypotheses=512, seed=0, min_inliers=16, max_error=1.0), **kw)
        want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
        assert want_model["valid"] == valid, (name, want_model)
        ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **kw)
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, len(fin))
        assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.epipolar_download(FB_M), want_out, want_model, name)
        assert ctx.featbuf_download(FB_IN, len(fin)).tobytes() == fin.tobytes()
        if valid != 1:
            assert want_out.tobytes() == fout.tobytes() and want_model["hypothesis"] == -1
    # n == 0: KLT_OK and nothing is written
    before_out, before_model = ctx.featbuf_download(FB_OUT, 20), ctx.epipolar_download(FB_M)
    ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, 0)
    ctx.sync()
    assert ctx.featbuf_download(FB_OUT, 20).tobytes() == before_out.tobytes() and ctx.epipolar_download(FB_M).tobytes() == before_model.tobytes()
    out, model, flagged = ctx.epipolar_check(fin64[:0], fout64[:0])
    assert len(out) == 0 and flagged == 0 and model.tobytes() == np.zeros((), EPIPOLAR_DTYPE).tobytes()


def test_a_second_call_gives_the_same_bytes(ctx):
    """the same lists uploaded again: the same bytes (nothing of a call survives in the scratch); the check called again on what it left: the
    rule on that (its flagged records are no candidates any more)"""
    fin, fout = mixed_lists(600, seed=77)
    kw = dict(hypotheses=64, seed=3, min_inliers=16, max_error=1.0)
    ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **kw)
    want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
    got = []
    for _ in range(2):
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, len(fin))
        got.append((ctx.featbuf_download(FB_OUT, len(fin)), ctx.epipolar_download(FB_M)))
        assert_same(got[-1][0], got[-1][1], want_out, want_model, "call %d" % len(got))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    again_out, again_model = epipolar_check_expected(fin, want_out, NCOLS, NROWS, **kw)
    ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, len(fin))
    assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.epipolar_download(FB_M), again_out, again_model, "the check on its own result")
    assert again_model["n_candidates"] == want_model["n_inliers"]


def test_a_batch_of_three_pairs_equals_three_single_calls(ctx):
    n = 300
    kw = dict(hypotheses=65, seed=3, min_inliers=16, max_error=1.0)
    ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **kw)
    lists = []
    for i in range(3):
        fin, fout, _ = parallax_n(n, NCOLS, NROWS, seed=70 + i)
        fout["val"][i * 40:i * 90] = -3                      # another number of candidates in every pair
        lists.append((fin, fout))
    assert len({int(candidate_mask(a, b, NCOLS, NROWS).sum()) for a, b in lists}) == 3
    pairs = []
    for i, (fin, fout) in enumerate(lists):
        ctx.featbuf_upload(200 + 3 * i, fin)
        ctx.featbuf_upload(201 + 3 * i, fout)
        pairs.append((200 + 3 * i, 201 + 3 * i, 202 + 3 * i))
    ctx.epipolar_check_batch_async(pairs, n)
    assert ctx.epipolar_check_path() == 2
    for i, (fin, fout) in enumerate(lists):
        want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
        assert want_model["valid"] == 1
        assert_same(ctx.featbuf_download(pairs[i][1], n), ctx.epipolar_download(pairs[i][2]), want_out, want_model, "pair %d of the batch" % i)
        single_out, single_model, _ = ctx.epipolar_check(fin, fout)
        assert_same(single_out, single_model, want_out, want_model, "pair %d alone" % i)
    from pyfeaturetrack_amd.backend import KltBackendError
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.epipolar_check_batch_async([pairs[0], (pairs[1][0], pairs[1][1], pairs[0][1])], n)       # a model buffer that is a list
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.epipolar_check_batch_async([pairs[0], (pairs[1][0], pairs[0][1], pairs[1][2])], n)       # two pairs rewrite one list
    fin, fout = lists[2]                                     # ... and the context works on
    ctx.featbuf_upload(pairs[2][1], fout)
    ctx.epipolar_check_batch_async([pairs[2]], n)
    want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
    assert_same(ctx.featbuf_download(pairs[2][1], n), ctx.epipolar_download(pairs[2][2]), want_out, want_model, "after the refused batches")


def test_error_returns_leave_the_context_working(ctx):
    from pyfeaturetrack_amd.backend import KltBackendError
    n = 64
    FB_IN, FB_OUT, FB_M, FB_VIEW = 110, 111, 112, 113       # buffers of this test's own: exactly n records each
    fin, fout, _ = parallax_n(n, NCOLS, NROWS, seed=5)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_OUT, fout)
    ctx.featbuf_view(FB_VIEW, FB_OUT, 0, n)
    ctx.set_epipolar_params(mode=0)
    for call in (lambda: ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, n), lambda: ctx.epipolar_check(fin, fout),
                 lambda: ctx.epipolar_check_batch_async([(FB_IN, FB_OUT, FB_M)], n)):
        with pytest.raises(KltBackendError, match="epipolar check is off"):
            call()
    kw = dict(hypotheses=64, seed=0, min_inliers=16, max_error=1.0)
    for bad in (dict(mode=2), dict(hypotheses=0), dict(hypotheses=65537), dict(min_inliers=7), dict(max_error=-1.0),
                dict(max_error=float("nan")), dict(ncols=0), dict(nrows=65536)):
        with pytest.raises(KltBackendError, match="epipolar"):
            ctx.set_epipolar_params(**dict(dict(ncols=NCOLS, nrows=NROWS, **kw), **bad))
    ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **kw)
    for args, pattern in (((FB_IN, FB_OUT, FB_OUT, n), "distinct"), ((FB_IN, FB_OUT, FB_IN, n), "distinct"), ((FB_IN, FB_IN, FB_M, n), "distinct"),
                          ((FB_IN, FB_OUT, FB_VIEW, n), "distinct"),                      # a view of fb_out: the same address under another index
                          ((FB_IN, FB_OUT, FB_M, n + 1), "not set"), ((FB_IN, 999, FB_M, n), "not set"), ((FB_IN, FB_OUT, FB_M, -1), "negative")):
        with pytest.raises(KltBackendError, match=pattern):
            ctx.epipolar_check_async(*args)
        ctx.sync()
        assert ctx.featbuf_download(FB_OUT, n).tobytes() == fout.tobytes() and ctx.featbuf_download(FB_IN, n).tobytes() == fin.tobytes()
    want_out, want_model = epipolar_check_expected(fin, fout, NCOLS, NROWS, **kw)
    ctx.epipolar_check_async(FB_IN, FB_OUT, FB_M, n)
    assert_same(ctx.featbuf_download(FB_OUT, n), ctx.epipolar_download(FB_M), want_out, want_model, "after the refused calls")


def test_the_motion_model_check_beside_it_keeps_its_own_scratch(ctx):
    """both checks on one context, alternating on the same lists: each equals its rule (they share the gather launch, not the scratch)"""
    from model_expected import motion_check_expected
    fin, fout, _ = parallax_n(300, NCOLS, NROWS, seed=91)
    ekw = dict(hypotheses=64, seed=1, min_inliers=16, max_error=1.0)
    mkw = dict(hypotheses=64, seed=1, min_inliers=8, max_error=1.0, min_area=1.0)
    ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **ekw)
    ctx.set_model_params(ncols=NCOLS, nrows=NROWS, **mkw)
    want_e, want_m = epipolar_check_expected(fin, fout, NCOLS, NROWS, **ekw), motion_check_expected(fin, fout, NCOLS, NROWS, **mkw)
    for _ in range(2):
        out, model, _ = ctx.epipolar_check(fin, fout)
        assert_same(out, model, want_e[0], want_e[1], "epipolar beside the motion model")
        out, model, _ = ctx.motion_check(fin, fout)
        assert out.tobytes() == want_m[0].tobytes() and np.asarray(model).tobytes() == want_m[1].tobytes()
    ctx.set_model_params(mode=0)


# ------------------------------------------------------------------------------------------------ Python API
_CLIP = {}
WINDOW, LEVELS, SS, NFEAT = 7, 2, 4, 150
MAX_ERROR = 0.5                          # px: the tracker's noise on the clip is a tenth of it, the moving block's step ten times it


def clip():
    if not _CLIP:
        _CLIP["frames"] = layered_clip()
    return _CLIP["frames"]


def _tc(**attrs):
    return make_tc(levels=LEVELS, ss=SS, window=WINDOW, **attrs)


def _load(ctx, frames):
    ctx.configure(_tc())
    ctx.set_light_params(mode=0)
    for k, f in enumerate(frames):
        ctx.upload(10 + k, f)
        ctx.build_pyramids(10 + k)


def _free(ctx, frames):
    for k in range(len(frames)):
        ctx.slot_free(10 + k)


def _quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    return old


def _restore(old):
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    sgf.KLT_verbose, tf.KLT_verbose = old


def _records(fl):
    a = np.zeros(len(fl), FEAT_DTYPE)
    a["x"], a["y"], a["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return a


def _same_xyv(got, want, what):
    for k in ("val", "x", "y"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, "%s.%s: %d differ, first at %d: got %r, want %r" % (what, k, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("sequential", [False, True], ids=["pingpong", "sequential"])
@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fb"])
def test_track_features_runs_the_check(ctx, sequential, fb):
    """KLTTrackFeatures with tc.epipolarCheck over three steps of the layered clip, lost features replaced after every step: the list it
    leaves is the plain (or forward-backward) tracker call on the records it held, then the rule; tc.epipolar_last is the rule's record.
    The block that moves down the columns is five pixels off every epipolar line: its features are flagged."""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = clip()
    old = _quiet()
    _load(ctx, frames)
    try:
        tc = _tc(sequentialMode=sequential, epipolarCheck=True, epipolar_seed=11, epipolar_max_error=MAX_ERROR, forwardBackwardCheck=fb,
                 trackQuality=True)
        kw = dict(hypotheses=512, seed=11, min_inliers=16, max_error=MAX_ERROR)
        fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
        flagged = flagged_inside = 0
        for k in range(1, 4):
            before = _records(fl)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            after = _records(fl)
            fwd = (ctx.track_fb if fb else ctx.track)(10 + k - 1, 10 + k, before)[0]
            want_out, want_model = epipolar_check_expected(before, fwd, NCOLS, NROWS, **kw)
            live = before["val"] >= 0
            _same_xyv(after[live], want_out[live], "step %d" % k)
            assert np.asarray(tc.epipolar_last).tobytes() == want_model.tobytes(), (tc.epipolar_last, want_model)
            flag = want_out["val"] == KLT_EPIPOLAR_OUTLIER
            inside = inside_mover(before, WINDOW) & live & (fwd["val"] == KLT_TRACKED)
            print("step %d: valid %d, %d candidates, %d flagged, %d of %d inside the moving block" % (k, want_model["valid"], want_model["n_candidates"],
                                                                                                  flag.sum(), (flag & inside).sum(), inside.sum()))
            assert want_model["valid"] == 1
            assert (tc.quality_last["val"][flag] == 0).all()                    # the quality launch runs behind the check
            flagged += int(flag.sum())
            flagged_inside += int((flag & inside).sum())
            KLTReplaceLostFeatures(tc, frames[k], fl)
        assert flagged_inside >= 5, (flagged, flagged_inside)
    finally:
        _restore(old)
        _free(ctx, frames)


@pytest.mark.parametrize("prefetch", [True, False])
def test_track_sequence_carries_the_records(ctx, prefetch):
    """KLTTrackSequence with tc.epipolarCheck, 6 frames, lost features replaced: row k of the table is the plain tracker call on row k - 1,
    then the rule, then the replacement pass, which refills flagged slots; ft.epipolar[k] is the rule's record, row 0 all zero"""
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = clip()
    old = _quiet()
    try:
        tc = _tc()
        plain = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        assert plain.epipolar is None and not (plain.rec["val"] == KLT_EPIPOLAR_OUTLIER).any()
        tc.epipolarCheck, tc.epipolar_max_error = True, MAX_ERROR
        ft = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        assert ft.models is None and ft.epipolar.shape == (len(frames),) and ft.epipolar.dtype == EPIPOLAR_DTYPE
        assert ft.epipolar[0].tobytes() == np.zeros((), EPIPOLAR_DTYPE).tobytes()
        assert np.array_equal(ft.rec[0], plain.rec[0])
        _load(ctx, frames)
        kw = dict(hypotheses=512, seed=0, min_inliers=16, max_error=MAX_ERROR)
        flagged = refilled = 0
        for k in range(1, len(frames)):
            before, after = np.ascontiguousarray(ft.rec[k - 1]), np.ascontiguousarray(ft.rec[k])
            fwd, _ = ctx.track(10 + k - 1, 10 + k, before)
            want_out, want_model = epipolar_check_expected(before, fwd, NCOLS, NROWS, **kw)
            assert ft.epipolar[k].tobytes() == want_model.tobytes(), (k, ft.epipolar[k], want_model)
            kept = after["val"] <= 0                                 # not refilled by frame k's replacement pass
            _same_xyv(after[kept], want_out[kept], "row %d" % k)
            flag = want_out["val"] == KLT_EPIPOLAR_OUTLIER
            flagged += int(flag.sum())
            refilled += int((flag & (after["val"] > 0)).sum())
            assert (want_out["val"][after["val"] > 0] < 0).all()     # only lost slots are refilled
        print("flagged %d over the clip, %d of them refilled on the same frame's replacement pass" % (flagged, refilled))
        assert flagged >= 5 and refilled >= 1, (flagged, refilled)
    finally:
        _restore(old)
        _free(ctx, frames)


def test_a_context_without_the_switch_enqueues_nothing():
    """a fresh context that never asks: klt_epipolar_check_path stays 0 through selection and tracking; through the Python API the path of
    the tracking context's device context does not move and the records are the plain call's"""
    from pyfeaturetrack_amd.backend import Context, context_of
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = clip()
    fresh = Context(0)
    try:
        _load(fresh, frames[:2])
        fin, _ = fresh.select(10, NFEAT, use_pyramid=True)
        fresh.track(10, 11, fin)
        assert fresh.epipolar_check_path() == 0
        old = _quiet()
        try:
            tc = _tc()
            path = context_of(tc).epipolar_check_path()
            fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
            fwd, _ = fresh.track(10, 11, _records(fl))
            KLTTrackFeatures(tc, frames[0], frames[1], fl)
            assert context_of(tc).epipolar_check_path() == path and not hasattr(tc, "epipolar_last")
            got = _records(fl)
            assert np.array_equal(got["x"], fwd["x"]) and np.array_equal(got["y"], fwd["y"]) and np.array_equal(got["val"], fwd["val"])
            assert not (got["val"] == KLT_EPIPOLAR_OUTLIER).any()
        finally:
            _restore(old)
    finally:
        fresh.close()
