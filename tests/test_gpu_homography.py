"""The homography check (klt_homography_check*) on the device against the numpy restatement of the rule
(tests/homography_expected.py), bit for bit on every byte of `out` and of the model record.  A difference is a bug in the kernels or in the
restatement's transcription of the rule, not a tolerance."""
import numpy as np
import pytest

from helpers import make_tc
from homography_expected import (HOMOGRAPHY_DTYPE, KLT_HOMOGRAPHY_OUTLIER, collinear_lists, homography_check_expected, homography_matrix,
                                 inside_mover, rotation_n, scene, warped_clip)
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
    got_model, want_model = np.asarray(got_model, HOMOGRAPHY_DTYPE).reshape(1), np.asarray(want_model, HOMOGRAPHY_DTYPE).reshape(1)
    assert got_model.tobytes() == want_model.tobytes(), "%s: model record differs: got %r, want %r" % (what, got_model[0], want_model[0])
    if got_out.tobytes() != want_out.tobytes():
        bad = np.flatnonzero((got_out.view(np.uint32).reshape(-1, 4) != want_out.view(np.uint32).reshape(-1, 4)).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, first at %d: got %r, want %r" % (what, bad.size, len(got_out), bad[0],
                                                                                            got_out[bad[0]], want_out[bad[0]]))


def mixed_lists(n, seed):
    """the rotation lists on the small frame; from 600 records on with every kind of non-candidate mixed in"""
    fin, fout, _ = rotation_n(n, NCOLS, NROWS, seed)
    if n >= 600:
        kinds = non_candidate_kinds(fin, fout, NCOLS, NROWS, start=1, step=max(1, n // 37))
        assert len(kinds) >= 30 and not candidate_mask(fin, fout, NCOLS, NROWS)[kinds].any()
    return fin, fout


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 64, 65, 600, 8193])
def test_kernels_equal_the_rule_across_counts(ctx, n):
    """n across the four picks, one wavefront, the 64 partials and several passes of the eight-wavefront stride (8193 > 4 * 512 * 4);
    hypotheses 1, 4 and 5 (the wavefronts of a scoring workgroup), 257 (inside one pass of the decide kernel's 512-thread argmax), 513 and
    1001 (past it: the strided loop of reduce_best_key takes a second trip); min_inliers 4 so that n = 4 can
    give a model and n = 3 none; every kind of non-candidate among the 600 and the 8193"""
    fin, fout = mixed_lists(n, seed=40 + n)
    seen = set()
    for hyp in (1, 4, 5, 257, 513, 1001):
        kw = dict(hypotheses=hyp, seed=7 * hyp, min_inliers=4 if n < 64 else 8, max_error=1.0)
        ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **kw)
        want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
        got_out, got_model, flagged = ctx.homography_check(fin, fout)
        assert_same(got_out, got_model, want_out, want_model, "n %d, %d hypotheses" % (n, hyp))
        assert flagged == int((want_out["val"] == KLT_HOMOGRAPHY_OUTLIER).sum()) - int((fout["val"] == KLT_HOMOGRAPHY_OUTLIER).sum())
        seen.add(int(want_model["valid"]))
        assert ctx.homography_check_path() == 1
    print("n %d: valid outcomes %r, last model %r" % (n, sorted(seen), want_model))
    assert seen == {0} if n < 4 else 1 in seen, seen
    if n >= 64:
        assert (want_out["val"] == KLT_HOMOGRAPHY_OUTLIER).any()


def test_the_rotation_scene_at_1080p(ctx):
    fin, fout, moved, _ = scene("rotation", 11)
    ctx.set_homography_params(ncols=1920, nrows=1080)        # the defaults
    want_out, want_model = homography_check_expected(fin, fout, 1920, 1080)
    got_out, got_model, flagged = ctx.homography_check(fin, fout)
    assert_same(got_out, got_model, want_out, want_model, "the rotation scene")
    flag = got_out["val"] == KLT_HOMOGRAPHY_OUTLIER
    assert got_model["valid"] == 1 and flagged == flag.sum()
    assert np.array_equal(flag, moved)                       # every static track kept, every displaced one flagged
    from pyfeaturetrack_amd.backend import homography_matrix as host_matrix
    assert np.array_equal(host_matrix(got_model), homography_matrix(want_model).reshape(3, 3))


def test_every_outcome_and_the_asynchronous_call(ctx):
    """valid 0 (too few candidates; every hypothesis singular; a best score below min_inliers) and 1 through klt_homography_check_async
    on resident lists (valid 2, a refit that fails, takes exact integer positions: tests/test_gpu_check_draws.py, entry `valid2`);
    collinear candidates; n = 0 enqueues nothing"""
    rs = np.random.RandomState(9)
    fin64, fout64, _ = rotation_n(64, NCOLS, NROWS, seed=5)
    k = np.arange(40)
    cin, cout = collinear_lists(40, NCOLS, NROWS, 3)
    cases = [("few", fin64[:7], fout64[:7], {}, 0),
             ("singular", records(16 + 7 * k, 30 + 3 * k), records(19 + 7 * k, 28 + 3 * k), {}, 0),
             ("no consensus", records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1),
              records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64)), dict(max_error=0.01, hypotheses=64), 0),
             ("noisy lists under 0.01 px", fin64, fout64, dict(max_error=0.01, hypotheses=64), 0),
             ("collinear", cin, cout, {}, None),
             ("refit", fin64, fout64, {}, 1)]
    for name, fin, fout, kw, valid in cases:
        kw = dict(dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0), **kw)
        want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
        assert valid is None or want_model["valid"] == valid, (name, want_model)
        ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **kw)
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.homography_check_async(FB_IN, FB_OUT, FB_M, len(fin))
        assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.homography_download(FB_M), want_out, want_model, name)
        assert ctx.featbuf_download(FB_IN, len(fin)).tobytes() == fin.tobytes()
        if valid == 0:
            assert want_out.tobytes() == fout.tobytes() and want_model["hypothesis"] == -1
        if name == "collinear":
            assert want_out.tobytes() == fout.tobytes()
    # n == 0: KLT_OK and nothing is written
    before_out, before_model = ctx.featbuf_download(FB_OUT, 20), ctx.homography_download(FB_M)
    ctx.homography_check_async(FB_IN, FB_OUT, FB_M, 0)
    ctx.sync()
    assert ctx.featbuf_download(FB_OUT, 20).tobytes() == before_out.tobytes() and ctx.homography_download(FB_M).tobytes() == before_model.tobytes()
    out, model, flagged = ctx.homography_check(fin64[:0], fout64[:0])
    assert len(out) == 0 and flagged == 0 and model.tobytes() == np.zeros((), HOMOGRAPHY_DTYPE).tobytes()


def test_a_second_call_gives_the_same_bytes(ctx):
    """the same lists uploaded again: the same bytes (nothing of a call survives in the scratch); the check called again on what it left: the
    rule on that (its flagged records are no candidates any more)"""
    fin, fout = mixed_lists(600, seed=77)
    kw = dict(hypotheses=64, seed=3, min_inliers=8, max_error=1.0)
    ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **kw)
    want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
    got = []
    for _ in range(2):
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.homography_check_async(FB_IN, FB_OUT, FB_M, len(fin))
        got.append((ctx.featbuf_download(FB_OUT, len(fin)), ctx.homography_download(FB_M)))
        assert_same(got[-1][0], got[-1][1], want_out, want_model, "call %d" % len(got))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    again_out, again_model = homography_check_expected(fin, want_out, NCOLS, NROWS, **kw)
    ctx.homography_check_async(FB_IN, FB_OUT, FB_M, len(fin))
    assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.homography_download(FB_M), again_out, again_model, "the check on its own result")
    assert again_model["n_candidates"] == want_model["n_inliers"]


def test_a_batch_of_three_pairs_equals_three_single_calls(ctx):
    n = 300
    kw = dict(hypotheses=65, seed=3, min_inliers=8, max_error=1.0)
    ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **kw)
    lists = []
    for i in range(3):
        fin, fout, _ = rotation_n(n, NCOLS, NROWS, seed=70 + i)
        fout["val"][i * 40:i * 90] = -3                      # another number of candidates in every pair
        lists.append((fin, fout))
    assert len({int(candidate_mask(a, b, NCOLS, NROWS).sum()) for a, b in lists}) == 3
    pairs = []
    for i, (fin, fout) in enumerate(lists):
        ctx.featbuf_upload(200 + 3 * i, fin)
        ctx.featbuf_upload(201 + 3 * i, fout)
        pairs.append((200 + 3 * i, 201 + 3 * i, 202 + 3 * i))
    ctx.homography_check_batch_async(pairs, n)
    assert ctx.homography_check_path() == 2
    for i, (fin, fout) in enumerate(lists):
        want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
        assert want_model["valid"] == 1
        assert_same(ctx.featbuf_download(pairs[i][1], n), ctx.homography_download(pairs[i][2]), want_out, want_model, "pair %d of the batch" % i)
        single_out, single_model, _ = ctx.homography_check(fin, fout)
        assert_same(single_out, single_model, want_out, want_model, "pair %d alone" % i)
    from pyfeaturetrack_amd.backend import KltBackendError
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.homography_check_batch_async([pairs[0], (pairs[1][0], pairs[1][1], pairs[0][1])], n)     # a model buffer that is a list
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.homography_check_batch_async([pairs[0], (pairs[1][0], pairs[0][1], pairs[1][2])], n)     # two pairs rewrite one list
    with pytest.raises(KltBackendError, match="bad argument"):
        ctx.homography_check_batch_async([pairs[0]], -1)
    fin, fout = lists[2]                                     # ... and the context works on
    ctx.featbuf_upload(pairs[2][1], fout)
    ctx.homography_check_batch_async([pairs[2]], n)
    want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
    assert_same(ctx.featbuf_download(pairs[2][1], n), ctx.homography_download(pairs[2][2]), want_out, want_model, "after the refused batches")


def test_error_returns_leave_the_context_working(ctx):
    from pyfeaturetrack_amd.backend import KltBackendError
    n = 64
    FB_IN, FB_OUT, FB_M, FB_VIEW = 110, 111, 112, 113       # buffers of this test's own: exactly n records each
    fin, fout, _ = rotation_n(n, NCOLS, NROWS, seed=5)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_OUT, fout)
    ctx.featbuf_view(FB_VIEW, FB_OUT, 0, n)
    ctx.set_homography_params(mode=0)
    for call in (lambda: ctx.homography_check_async(FB_IN, FB_OUT, FB_M, n), lambda: ctx.homography_check(fin, fout),
                 lambda: ctx.homography_check_batch_async([(FB_IN, FB_OUT, FB_M)], n)):
        with pytest.raises(KltBackendError, match="homography check is off"):
            call()
    kw = dict(hypotheses=64, seed=0, min_inliers=8, max_error=1.0)
    for bad in (dict(mode=2), dict(mode=-1), dict(hypotheses=0), dict(hypotheses=65537), dict(min_inliers=3), dict(max_error=-1.0),
                dict(max_error=float("nan")), dict(ncols=0), dict(nrows=65536)):
        with pytest.raises(KltBackendError, match="homography"):
            ctx.set_homography_params(**dict(dict(ncols=NCOLS, nrows=NROWS, **kw), **bad))
    ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **kw)
    for args, pattern in (((FB_IN, FB_OUT, FB_OUT, n), "distinct"), ((FB_IN, FB_OUT, FB_IN, n), "distinct"), ((FB_IN, FB_IN, FB_M, n), "distinct"),
                          ((FB_IN, FB_OUT, FB_VIEW, n), "distinct"),                      # a view of fb_out: the same address under another index
                          ((FB_IN, FB_OUT, FB_M, n + 1), "not set"), ((FB_IN, 999, FB_M, n), "not set"), ((FB_IN, FB_OUT, FB_M, -1), "negative")):
        with pytest.raises(KltBackendError, match=pattern):
            ctx.homography_check_async(*args)
        ctx.sync()
        assert ctx.featbuf_download(FB_OUT, n).tobytes() == fout.tobytes() and ctx.featbuf_download(FB_IN, n).tobytes() == fin.tobytes()
    want_out, want_model = homography_check_expected(fin, fout, NCOLS, NROWS, **kw)
    ctx.homography_check_async(FB_IN, FB_OUT, FB_M, n)
    assert_same(ctx.featbuf_download(FB_OUT, n), ctx.homography_download(FB_M), want_out, want_model, "after the refused calls")
    # the other two setters keep refusing mode 2
    for setter in (ctx.set_model_params, ctx.set_epipolar_params):
        with pytest.raises(KltBackendError):
            setter(mode=2, ncols=NCOLS, nrows=NROWS)


def test_all_three_checks_on_one_context_keep_their_own_scratch(ctx):
    """the three checks on one context, alternating on the same lists, each into a model buffer of its own: each equals its rule and leaves
    the other two records alone (they share the gather launch, not the scratch)"""
    from epipolar_expected import epipolar_check_expected
    from model_expected import motion_check_expected
    fin, fout, _ = rotation_n(300, NCOLS, NROWS, seed=91)
    hkw = dict(hypotheses=64, seed=1, min_inliers=8, max_error=1.0)
    ekw = dict(hypotheses=64, seed=1, min_inliers=16, max_error=1.0)
    mkw = dict(hypotheses=64, seed=1, min_inliers=8, max_error=1.0, min_area=1.0)
    ctx.set_homography_params(ncols=NCOLS, nrows=NROWS, **hkw)
    ctx.set_epipolar_params(ncols=NCOLS, nrows=NROWS, **ekw)
    ctx.set_model_params(ncols=NCOLS, nrows=NROWS, **mkw)
    want_h = homography_check_expected(fin, fout, NCOLS, NROWS, **hkw)
    want_e, want_m = epipolar_check_expected(fin, fout, NCOLS, NROWS, **ekw), motion_check_expected(fin, fout, NCOLS, NROWS, **mkw)
    FB_H, FB_E, FB_MM = 120, 121, 122
    ctx.featbuf_upload(FB_IN, fin)
    for _ in range(2):
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.homography_check_async(FB_IN, FB_OUT, FB_H, len(fin))
        assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.homography_download(FB_H), want_h[0], want_h[1], "homography beside the others")
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.epipolar_check_async(FB_IN, FB_OUT, FB_E, len(fin))
        assert ctx.featbuf_download(FB_OUT, len(fin)).tobytes() == want_e[0].tobytes()
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.motion_check_async(FB_IN, FB_OUT, FB_MM, len(fin))
        assert ctx.featbuf_download(FB_OUT, len(fin)).tobytes() == want_m[0].tobytes()
        assert np.asarray(ctx.homography_download(FB_H)).tobytes() == want_h[1].tobytes()
        assert np.asarray(ctx.epipolar_download(FB_E)).tobytes() == want_e[1].tobytes()
        assert np.asarray(ctx.model_download(FB_MM)).tobytes() == want_m[1].tobytes()
    ctx.set_model_params(mode=0)
    ctx.set_epipolar_params(mode=0)


# ------------------------------------------------------------------------------------------------ Python API
_CLIP = {}
WINDOW, LEVELS, SS, NFEAT = 7, 2, 4, 150
MAX_ERROR = 0.5                          # px: the tracker's noise on the clip is a fraction of it, the moving block is several px off


def clip():
    if not _CLIP:
        _CLIP["frames"] = warped_clip()
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
    """KLTTrackFeatures with tc.homographyCheck over three steps of the warped clip, lost features replaced after every step: the list it
    leaves is the plain (or forward-backward) tracker call on the records it held, then the rule; tc.homography_last is the rule's record.
    The block that moves down the columns on its own is off the background's homography: its features are flagged."""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = clip()
    old = _quiet()
    _load(ctx, frames)
    try:
        tc = _tc(sequentialMode=sequential, homographyCheck=True, homography_seed=11, homography_max_error=MAX_ERROR, forwardBackwardCheck=fb,
                 trackQuality=True)
        kw = dict(hypotheses=256, seed=11, min_inliers=8, max_error=MAX_ERROR)
        fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
        for k in range(1, 4):
            before = _records(fl)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            after = _records(fl)
            fwd = (ctx.track_fb if fb else ctx.track)(10 + k - 1, 10 + k, before)[0]
            want_out, want_model = homography_check_expected(before, fwd, NCOLS, NROWS, **kw)
            live = before["val"] >= 0
            _same_xyv(after[live], want_out[live], "step %d" % k)
            assert np.asarray(tc.homography_last).tobytes() == want_model.tobytes(), (tc.homography_last, want_model)
            flag = want_out["val"] == KLT_HOMOGRAPHY_OUTLIER
            inside = inside_mover(before, WINDOW) & live & (fwd["val"] == KLT_TRACKED)
            print("step %d: valid %d, %d candidates, %d flagged, %d of %d inside the moving block" % (k, want_model["valid"], want_model["n_candidates"],
                                                                                                  flag.sum(), (flag & inside).sum(), inside.sum()))
            assert want_model["valid"] == 1
            assert inside.sum() >= 3 and flag[inside].all()                     # every tracked feature wholly inside the block
            assert (tc.quality_last["val"][flag] == 0).all()                    # the quality launch runs behind the check
            KLTReplaceLostFeatures(tc, frames[k], fl)
    finally:
        _restore(old)
        _free(ctx, frames)


@pytest.mark.parametrize("prefetch", [True, False])
def test_track_sequence_carries_the_records(ctx, prefetch):
    """KLTTrackSequence with tc.homographyCheck, 6 frames, lost features replaced: row k of the table is the plain tracker call on row
    k - 1, then the rule, then the replacement pass; ft.homography[k] is the rule's record, row 0 all zero.  Every tracked feature wholly
    inside the moving block is flagged in every step, and every flagged slot is refilled by the same frame's replacement pass."""
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = clip()
    old = _quiet()
    try:
        tc = _tc()
        plain = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        assert plain.homography is None and not (plain.rec["val"] == KLT_HOMOGRAPHY_OUTLIER).any()
        tc.homographyCheck, tc.homography_max_error = True, MAX_ERROR
        ft = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        assert ft.models is None and ft.epipolar is None
        assert ft.homography.shape == (len(frames),) and ft.homography.dtype == HOMOGRAPHY_DTYPE
        assert ft.homography[0].tobytes() == np.zeros((), HOMOGRAPHY_DTYPE).tobytes()
        assert np.array_equal(ft.rec[0], plain.rec[0])
        _load(ctx, frames)
        kw = dict(hypotheses=256, seed=0, min_inliers=8, max_error=MAX_ERROR)
        flagged = 0
        for k in range(1, len(frames)):
            before, after = np.ascontiguousarray(ft.rec[k - 1]), np.ascontiguousarray(ft.rec[k])
            fwd, _ = ctx.track(10 + k - 1, 10 + k, before)
            want_out, want_model = homography_check_expected(before, fwd, NCOLS, NROWS, **kw)
            assert ft.homography[k].tobytes() == want_model.tobytes(), (k, ft.homography[k], want_model)
            assert want_model["valid"] == 1
            kept = after["val"] <= 0                                 # not refilled by frame k's replacement pass
            _same_xyv(after[kept], want_out[kept], "row %d" % k)
            flag = want_out["val"] == KLT_HOMOGRAPHY_OUTLIER
            inside = inside_mover(before, WINDOW) & (before["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
            print("row %d: %d flagged, %d of %d inside the moving block, %d of the flagged refilled" % (
                k, flag.sum(), (flag & inside).sum(), inside.sum(), (flag & (after["val"] > 0)).sum()))
            assert inside.sum() >= 3 and flag[inside].all()
            assert (after["val"][flag] > 0).all()                    # every flagged slot is refilled on the same frame
            assert (want_out["val"][after["val"] > 0] < 0).all()     # only lost slots are refilled
            flagged += int(flag.sum())
        assert flagged >= 5 * 3
    finally:
        _restore(old)
        _free(ctx, frames)


def test_a_context_without_the_switch_enqueues_nothing():
    """a fresh context that never asks: klt_homography_check_path stays 0 through selection and tracking; through the Python API the path
    of the tracking context's device context does not move and the records are the plain call's"""
    from pyfeaturetrack_amd.backend import Context, context_of
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = clip()
    fresh = Context(0)
    try:
        _load(fresh, frames[:2])
        fin, _ = fresh.select(10, NFEAT, use_pyramid=True)
        fresh.track(10, 11, fin)
        assert fresh.homography_check_path() == 0
        old = _quiet()
        try:
            tc = _tc()
            path = context_of(tc).homography_check_path()
            fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
            fwd, _ = fresh.track(10, 11, _records(fl))
            KLTTrackFeatures(tc, frames[0], frames[1], fl)
            assert context_of(tc).homography_check_path() == path and not hasattr(tc, "homography_last")
            got = _records(fl)
            assert np.array_equal(got["x"], fwd["x"]) and np.array_equal(got["y"], fwd["y"]) and np.array_equal(got["val"], fwd["val"])
            assert not (got["val"] == KLT_HOMOGRAPHY_OUTLIER).any()
        finally:
            _restore(old)
    finally:
        fresh.close()
