"""The crowding check through the Python API (tc.crowdingCheck) on a zoom-out clip: KLTTrackFeatures and
KLTTrackSequence against the step-by-step composition through the context's primitives (track, check, replace) and the rule's plain
restatement (tests/crowd_expected.py).  Comparisons are on bytes (x, y, val: the Python lists carry no aux)."""
import numpy as np
import pytest

from crowd_expected import CROWD_DTYPE, FEAT_DTYPE, KLT_CROWDED, crowd_check_expected, crowd_records, live_pairs_within, zoom_out_clip
from helpers import make_tc

pytestmark = pytest.mark.gpu

NCOLS, NROWS = 320, 240
WINDOW, LEVELS, SS, NFEAT = 7, 2, 4, 300
_CLIP = {}


def clip():
    if not _CLIP:
        _CLIP["frames"] = zoom_out_clip(12, NCOLS, NROWS)
    return _CLIP["frames"]


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


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
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, "%s.%s: %d differ, first at %d: got %r, want %r" % (what, k, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _same_crowd(got, want, what):
    got, want = np.ascontiguousarray(got).view(CROWD_DTYPE), np.ascontiguousarray(want)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1))
        raise AssertionError("%s: %d crowd records differ, first at %d: got %r, want %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]]))


DIST = 14                                # the pair's own distance, past tc.mindist = 10: one zoom-out step then collides for sure


@pytest.mark.parametrize("sequential", [False, True], ids=["pingpong", "sequential"])
def test_track_features_runs_the_check_and_honours_age(ctx, sequential):
    """KLTTrackFeatures with tc.crowdingCheck on a zoom-out pair: the list it leaves is the plain tracker call's records with the rule
    applied, tc.crowding_last the rule's records; without `age` list order decides, with it the older track stays: reversed ages flip
    which of two colliding tracks survives; the quality launch runs behind the check"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = clip()
    old = _quiet()
    _load(ctx, frames[:2])
    try:
        n = NFEAT
        rising = np.arange(n, dtype=np.int32)
        outcomes = {}
        for name, age in (("none", None), ("rising", rising), ("falling", rising[::-1].copy())):
            tc = _tc(sequentialMode=sequential, crowdingCheck=True, crowding_min_distance=DIST, trackQuality=True)
            fl = KLTSelectGoodFeatures(tc, frames[0], n)
            before = _records(fl)
            KLTTrackFeatures(tc, frames[0], frames[1], fl, age=age)
            after = _records(fl)
            fwd = ctx.track(10, 11, before)[0]
            want_out, want_crowd = crowd_check_expected(fwd, None if age is None else crowd_records(age), NCOLS, NROWS, DIST)
            live = before["val"] >= 0
            assert live.sum() >= 200
            _same_xyv(after[live], want_out[live], "ages %s" % name)
            _same_crowd(tc.crowding_last, want_crowd, "ages %s" % name)
            flagged = want_crowd["val"] == 2
            print("ages %s: %d tracked, %d crowded" % (name, (fwd["val"] == 0).sum(), flagged.sum()))
            assert flagged.sum() >= 5 and (after["val"][flagged] == KLT_CROWDED).all()
            assert live_pairs_within(after, DIST - 1, NCOLS, NROWS) == 0 and live_pairs_within(fwd, DIST - 1, NCOLS, NROWS) > 0
            assert (tc.quality_last["val"][flagged] == 0).all()
            outcomes[name] = want_crowd
        # no ages: list order decides, as ages falling along the list do; rising ages decide otherwise
        assert outcomes["none"]["winner"].tobytes() == outcomes["falling"]["winner"].tobytes()
        assert outcomes["none"]["val"].tobytes() != outcomes["rising"]["val"].tobytes()
        # a pair of colliding tracks whose survivor the ages decide: i loses to w under rising ages, w to i under falling ones
        up, down = outcomes["rising"], outcomes["falling"]
        flips = [i for i in np.flatnonzero(up["val"] == 2) if down["val"][i] == 1 and down["val"][up["winner"][i]] == 2
                 and down["winner"][up["winner"][i]] == i]
        assert flips, "no pair of colliding tracks changed its survivor with the ages"
        assert all(up["winner"][i] > i for i in flips)       # rising ages: the higher index is the older track
    finally:
        _restore(old)
        _free(ctx, frames[:2])


def test_bad_arguments_raise_before_any_device_work():
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = clip()
    old = _quiet()
    try:
        for attrs in (dict(crowdingCheck=1), dict(crowdingCheck=True, crowding_min_distance=0),
                      dict(crowdingCheck=True, affineConsistencyCheck=0)):
            tc = _tc(**attrs)
            with pytest.raises(ValueError):
                KLTTrackFeatures(tc, frames[0], frames[1], [])
            with pytest.raises(ValueError):
                KLTTrackSequence(tc, frames[:2], 10)
            assert "_klt_ctx" not in tc.__dict__
        with pytest.raises(ValueError):
            KLTTrackFeatures(_tc(crowdingCheck=True), frames[0], frames[1], [], age=[1, 2])
    finally:
        _restore(old)


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "plain"])
def test_track_sequence_keeps_the_live_features_apart(ctx, prefetch):
    """KLTTrackSequence over the 12 zoom-out frames, 300 features, lost ones replaced: row k of the table is the tracker on row k - 1, then
    the rule with row k - 1 of ft.crowd, then the replacement pass; ft.crowd[k] is the rule's records; after every frame no two live
    features are within r.  The same clip with the check off does have such pairs, never reports KLT_CROWDED, enqueues no crowd launch."""
    from pyfeaturetrack_amd.backend import REPLACING_SOME, Context
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = clip()
    old = _quiet()
    fresh = Context(0)                                       # a context of this test's own: nothing has asked it for the check yet
    try:
        tc = _tc()
        tc.__dict__["_klt_ctx"] = fresh
        r = tc.mindist - 1
        fresh.timing_enable(True)
        plain = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        names = [t["name"] for t in fresh.timing_read()]
        assert fresh.crowd_check_path() == 0 and names and not any("crowd" in name for name in names), names
        assert plain.crowd is None and not (plain.rec["val"] == KLT_CROWDED).any()
        pairs = [live_pairs_within(np.ascontiguousarray(row), r, NCOLS, NROWS) for row in plain.rec]
        print("check off: live pairs within %d px per frame: %r" % (r, pairs))
        assert pairs[0] == 0 and pairs[-1] > 0 and sum(pairs) >= 20
        tc.crowdingCheck = True
        ft = KLTTrackSequence(tc, frames, NFEAT, prefetch=prefetch)
        names = [t["name"] for t in fresh.timing_read()]
        assert fresh.crowd_check_path() == 1 and "crowd_check" in names and "crowd_prepare" in names
        fresh.timing_enable(False)
        assert ft.crowd.shape == (len(frames), NFEAT) and ft.crowd.dtype == CROWD_DTYPE
        assert ft.crowd[0].tobytes() == np.zeros(NFEAT, CROWD_DTYPE).tobytes()
        assert np.array_equal(ft.rec[0], plain.rec[0])
        _load(ctx, frames)
        ctx.set_crowd_params(ncols=NCOLS, nrows=NROWS, min_distance=tc.mindist)
        crowded, worst = 0, 0
        for k in range(1, len(frames)):
            before, after = np.ascontiguousarray(ft.rec[k - 1]), np.ascontiguousarray(ft.rec[k])
            fwd, _ = ctx.track(10 + k - 1, 10 + k, before)
            prev = np.ascontiguousarray(ft.crowd[k - 1])
            want_out, want_crowd = crowd_check_expected(fwd, prev, NCOLS, NROWS, tc.mindist)
            got_out, got_crowd, count = ctx.crowd_check(fwd, prev)                    # the context's own primitive says the same
            worst = max(worst, ctx.crowd_check_rounds())
            assert got_out.tobytes() == want_out.tobytes()
            _same_crowd(got_crowd, want_crowd, "the primitive, row %d" % k)
            _same_crowd(ft.crowd[k], want_crowd, "ft.crowd[%d]" % k)
            replaced, _ = ctx.select(10 + k, NFEAT, mode=REPLACING_SOME, fl=want_out, use_pyramid=True)
            _same_xyv(after, replaced, "row %d" % k)
            assert live_pairs_within(after, r, NCOLS, NROWS) == 0
            flag = want_crowd["val"] == 2
            print("row %d: %d tracked, %d crowded, %d of them refilled, oldest track %d" % (
                k, (fwd["val"] == 0).sum(), flag.sum(), (after["val"][flag] > 0).sum(), want_crowd["age"].max()))
            assert (want_out["val"][after["val"] > 0] < 0).all()     # only lost slots are refilled
            crowded += int(flag.sum())
        print("worst round count of the sequence: %d" % worst)
        assert crowded >= 20 and ft.crowd["age"].max() >= 6          # tracks that live through the clip grow older row by row
    finally:
        _restore(old)
        _free(ctx, frames)
        fresh.close()
