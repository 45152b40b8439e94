"""The motion-model check (klt_motion_check*) on the device against the numpy restatement of the rule
(tests/model_expected.py), bit for bit on every byte of `out` and of the model record.  A difference is a bug in the kernels or in the
restatement's transcription of the rule, not a tolerance."""
import numpy as np
import pytest

from fb_expected import OCCLUSION_CASES
from helpers import make_tc
from model_expected import (BLOCK_MOTION, FEAT_DTYPE, KLT_MODEL_OUTLIER, KLT_TRACKED, MODEL_DTYPE, block_sides, candidate_mask,
                            model_affine, motion_check_expected, moving_block_pair, non_candidate_kinds, records, synthetic_lists)

pytestmark = pytest.mark.gpu

FB_IN, FB_OUT, FB_M = 100, 101, 102


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_same(got_out, got_model, want_out, want_model, what):
    """bytes: the lists hold NaN coordinates, and -0 is not +0"""
    got_model, want_model = np.asarray(got_model, MODEL_DTYPE).reshape(1), np.asarray(want_model, MODEL_DTYPE).reshape(1)
    assert got_model.tobytes() == want_model.tobytes(), "%s: model record differs: got %r, want %r" % (what, got_model[0], want_model[0])
    if got_out.tobytes() != want_out.tobytes():
        bad = np.flatnonzero((got_out.view(np.uint32).reshape(-1, 4) != want_out.view(np.uint32).reshape(-1, 4)).any(axis=1))
        raise AssertionError("%s: %d of %d records differ, first at %d: got %r, want %r" % (what, bad.size, len(got_out), bad[0],
                                                                                            got_out[bad[0]], want_out[bad[0]]))


def mixed_lists(n, ncols, nrows, seed):
    """the synthetic lists; from 300 records on with every kind of non-candidate mixed in"""
    fin, fout, _, _, _ = synthetic_lists(n, ncols, nrows, seed)
    if n >= 300:
        non_candidate_kinds(fin, fout, ncols, nrows, start=1, step=max(1, n // 37))
    return fin, fout


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 300, 4097])
def test_kernels_equal_the_rule_on_synthetic_lists(ctx, n):
    """n across the wavefront, the workgroup and one tile of the gather; hypotheses 1, 5, 256 and 1001 (not a multiple of the four
    wavefronts of a scoring workgroup); min_inliers 3 so that n = 3 gives a model and n = 1 none"""
    ncols, nrows = (1920, 1080) if n != 65 else (4096, 2160)
    fin, fout = mixed_lists(n, ncols, nrows, seed=40 + n)
    seen = set()
    for hyp in (1, 5, 256, 1001):
        kw = dict(hypotheses=hyp, seed=7 * hyp, min_inliers=3, max_error=0.5, min_area=1.0)
        ctx.set_model_params(ncols=ncols, nrows=nrows, **kw)
        want_out, want_model = motion_check_expected(fin, fout, ncols, nrows, **kw)
        got_out, got_model, flagged = ctx.motion_check(fin, fout)
        assert_same(got_out, got_model, want_out, want_model, "n %d, %d hypotheses" % (n, hyp))
        assert flagged == int((want_out["val"] == KLT_MODEL_OUTLIER).sum()) - int((fout["val"] == KLT_MODEL_OUTLIER).sum())
        seen.add(int(want_model["valid"]))
        assert ctx.motion_check_path() == 1
    print("n %d: valid outcomes %r, last model %r" % (n, sorted(seen), want_model))
    assert seen == {0} if n == 1 else 1 in seen, seen
    if n in (63, 64, 65):                                    # (1001 hypotheses) exactly the displaced quarter
        assert want_model["valid"] == 1 and (want_out["val"] == KLT_MODEL_OUTLIER).sum() == n // 4


def test_every_outcome_and_the_asynchronous_call(ctx):
    """valid 0 (too few candidates; every area 0; a best score below min_inliers), 1 and 2 (min_area 0 on collinear integer positions:
    an exact determinant 0) through klt_motion_check_async on resident lists; n = 0 enqueues nothing"""
    ncols, nrows = 320, 240
    x = np.arange(40, dtype=np.float64) * 5 + 20
    rs = np.random.RandomState(9)
    fin64, fout64, _, _, _ = synthetic_lists(64, ncols, nrows, seed=5)
    cases = [("few", fin64[:7], fout64[:7], {}, 0),
             ("collinear", records(x, 0.5 * x + 10, 3), records(x + 1, 0.5 * x + 11), {}, 0),
             ("no consensus", records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1),
              records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64)), dict(max_error=0.01), 0),
             ("refit", fin64, fout64, dict(max_error=0.5), 1),
             ("kept hypothesis", records(x[:20] + 20, x[:20] + 28, 1), records(x[:20] + 22, x[:20] + 30), dict(min_area=0.0, hypotheses=5), 2)]
    for name, fin, fout, kw, valid in cases:
        kw = dict(dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0, min_area=1.0), **kw)
        want_out, want_model = motion_check_expected(fin, fout, ncols, nrows, **kw)
        assert want_model["valid"] == valid, (name, want_model)
        ctx.set_model_params(ncols=ncols, nrows=nrows, **kw)
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.motion_check_async(FB_IN, FB_OUT, FB_M, len(fin))
        assert_same(ctx.featbuf_download(FB_OUT, len(fin)), ctx.model_download(FB_M), want_out, want_model, name)
        assert ctx.featbuf_download(FB_IN, len(fin)).tobytes() == fin.tobytes()
        if valid != 1:
            assert want_out.tobytes() == fout.tobytes()
    # n == 0: KLT_OK and nothing is written
    before_out, before_model = ctx.featbuf_download(FB_OUT, 20), ctx.model_download(FB_M)
    ctx.motion_check_async(FB_IN, FB_OUT, FB_M, 0)
    ctx.sync()
    assert ctx.featbuf_download(FB_OUT, 20).tobytes() == before_out.tobytes() and ctx.model_download(FB_M).tobytes() == before_model.tobytes()
    out, model, flagged = ctx.motion_check(fin64[:0], fout64[:0])
    assert len(out) == 0 and flagged == 0 and model.tobytes() == np.zeros((), MODEL_DTYPE).tobytes()


def test_a_batch_of_three_pairs_equals_three_single_calls(ctx):
    ncols, nrows, n = 1920, 1080, 300
    kw = dict(hypotheses=256, seed=3, min_inliers=8, max_error=0.5, min_area=1.0)
    ctx.set_model_params(ncols=ncols, nrows=nrows, **kw)
    lists = []
    for i in range(3):
        fin, fout = mixed_lists(n, ncols, nrows, seed=70 + i)
        fout["val"][i * 40:i * 90] = -3                      # another number of candidates in every pair
        lists.append((fin, fout))
    assert len({int(candidate_mask(a, b, ncols, nrows).sum()) for a, b in lists}) == 3
    pairs = []
    for i, (fin, fout) in enumerate(lists):
        ctx.featbuf_upload(200 + 3 * i, fin)
        ctx.featbuf_upload(201 + 3 * i, fout)
        pairs.append((200 + 3 * i, 201 + 3 * i, 202 + 3 * i))
    ctx.motion_check_batch_async(pairs, n)
    assert ctx.motion_check_path() == 2
    for i, (fin, fout) in enumerate(lists):
        want_out, want_model = motion_check_expected(fin, fout, ncols, nrows, **kw)
        assert_same(ctx.featbuf_download(pairs[i][1], n), ctx.model_download(pairs[i][2]), want_out, want_model, "pair %d of the batch" % i)
        single_out, single_model, _ = ctx.motion_check(fin, fout)
        assert_same(single_out, single_model, want_out, want_model, "pair %d alone" % i)
    from pyfeaturetrack_amd.backend import KltBackendError
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.motion_check_batch_async([pairs[0], (pairs[1][0], pairs[1][1], pairs[0][1])], n)       # a model buffer that is a list
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.motion_check_batch_async([pairs[0], (pairs[1][0], pairs[0][1], pairs[1][2])], n)       # two pairs rewrite one list


# ---------------------------------------------------------------------------------------------------- frames: the moving block
_BLOCK = {}


def block_case():
    """the 320x240 7x7 moving-block geometry as a clip of 6 frames: background k * (1.3, -0.8), the block's texture k * BLOCK_MOTION"""
    if not _BLOCK:
        from pyfeaturetrack_amd import synth
        name, width, height, window, levels, ss, block, n = OCCLUSION_CASES[0]
        base, other = synth.synth_base(width, height, 21), synth.synth_base(width, height, 22)
        y0, y1, x0, x1 = block
        frames = []
        for k in range(6):
            f = synth.shift_frame(base, 1.3 * k, -0.8 * k)
            f[y0:y1, x0:x1] = synth.shift_frame(other, BLOCK_MOTION[0] * k, BLOCK_MOTION[1] * k)[y0:y1, x0:x1]
            f.setflags(write=False)
            frames.append(f)
        pair = moving_block_pair(width, height, block)
        assert np.array_equal(pair[0], frames[0]) and np.array_equal(pair[1], frames[1])
        _BLOCK.update(frames=frames, size=(width, height), window=window, levels=levels, ss=ss, block=block, n=n)
    return _BLOCK


def _tc(c, **attrs):
    return make_tc(levels=c["levels"], ss=c["ss"], window=c["window"], **attrs)


def _load(ctx, c):
    ctx.configure(_tc(c))
    ctx.set_light_params(mode=0)
    for k, f in enumerate(c["frames"]):
        ctx.upload(10 + k, f)
        ctx.build_pyramids(10 + k)


def _free(ctx, c):
    for k in range(len(c["frames"])):
        ctx.slot_free(10 + k)


def test_the_moving_block_with_lists_from_the_device_tracker(ctx):
    c = block_case()
    ncols, nrows = c["size"]
    _load(ctx, c)
    try:
        fin, placed = ctx.select(10, c["n"], use_pyramid=True)
        fwd, _ = ctx.track(10, 11, fin)
        fb_out, _ = ctx.track_fb(10, 11, fin)
        kw = dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0, min_area=1.0)
        ctx.set_model_params(ncols=ncols, nrows=nrows, **kw)
        got_out, got_model, flagged = ctx.motion_check(fin, fwd)
        want_out, want_model = motion_check_expected(fin, fwd, ncols, nrows, **kw)
        assert_same(got_out, got_model, want_out, want_model, "the moving block")
        tracked = (fin["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
        inside, outside = block_sides(fin, c["block"], c["window"])
        flag = got_out["val"] == KLT_MODEL_OUTLIER
        print("tracked %d, inside %d (%d flagged), outside %d (%d flagged), flagged and kept by the forward-backward check %d"
              % (tracked.sum(), (tracked & inside).sum(), (flag & inside).sum(), (tracked & outside).sum(), (flag & outside).sum(),
                 (flag & (fb_out["val"] == KLT_TRACKED)).sum()))
        assert (tracked & inside).sum() >= 10 and flag[tracked & inside].all() and not flag[tracked & outside].any()
        assert (flag & (fb_out["val"] == KLT_TRACKED)).any()
        from pyfeaturetrack_amd.backend import model_affine as host_affine
        A, t = host_affine(got_model)
        A2, t2 = model_affine(want_model)
        assert np.array_equal(A, A2) and np.array_equal(t, t2) and abs(t[0] - 1.3) < 0.5 and abs(t[1] + 0.8) < 0.5
    finally:
        _free(ctx, c)


def test_error_returns_leave_the_context_working(ctx):
    from pyfeaturetrack_amd.backend import KltBackendError
    c = block_case()
    ncols, nrows = c["size"]
    n = 64
    fin, fout, _, _, _ = synthetic_lists(n, ncols, nrows, seed=5)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_OUT, fout)
    ctx.featbuf_view(103, FB_OUT, 0, n)
    ctx.set_model_params(mode=0)
    for call in (lambda: ctx.motion_check_async(FB_IN, FB_OUT, FB_M, n), lambda: ctx.motion_check(fin, fout),
                 lambda: ctx.motion_check_batch_async([(FB_IN, FB_OUT, FB_M)], n)):
        with pytest.raises(KltBackendError, match="motion-model check is off"):
            call()
    kw = dict(hypotheses=256, seed=0, min_inliers=8, max_error=0.5, min_area=1.0)
    for bad in (dict(mode=2), dict(hypotheses=0), dict(hypotheses=65537), dict(min_inliers=2), dict(max_error=-1.0),
                dict(max_error=float("nan")), dict(min_area=-1.0), dict(ncols=0), dict(nrows=65536)):
        with pytest.raises(KltBackendError, match="motion.model"):
            ctx.set_model_params(**dict(dict(ncols=ncols, nrows=nrows, **kw), **bad))
    ctx.set_model_params(ncols=ncols, nrows=nrows, **kw)
    for args, pattern in (((FB_IN, FB_OUT, FB_OUT, n), "distinct"), ((FB_IN, FB_OUT, FB_IN, n), "distinct"), ((FB_IN, FB_IN, FB_M, n), "distinct"),
                          ((FB_IN, FB_OUT, 103, n), "distinct"),                      # a view of fb_out: the same address under another index
                          ((FB_IN, FB_OUT, FB_M, n + 1), "not set"), ((FB_IN, 999, FB_M, n), "not set"), ((FB_IN, FB_OUT, FB_M, -1), "negative")):
        with pytest.raises(KltBackendError, match=pattern):
            ctx.motion_check_async(*args)
        ctx.sync()
        assert ctx.featbuf_download(FB_OUT, n).tobytes() == fout.tobytes() and ctx.featbuf_download(FB_IN, n).tobytes() == fin.tobytes()
    want_out, want_model = motion_check_expected(fin, fout, ncols, nrows, **kw)
    ctx.motion_check_async(FB_IN, FB_OUT, FB_M, n)
    assert_same(ctx.featbuf_download(FB_OUT, n), ctx.model_download(FB_M), want_out, want_model, "after the refused calls")
    _load(ctx, c)                                            # ... and the context tracks on
    try:
        sel, placed = ctx.select(10, 50, use_pyramid=True)
        out, tracked = ctx.track(10, 11, sel)
        assert placed == 50 and tracked >= 30
    finally:
        _free(ctx, c)


def test_a_context_without_the_switch_enqueues_nothing():
    """a fresh context that never asks: klt_motion_check_path stays 0 through selection and tracking; through the Python API the path of
    the tracking context's device context does not move and the records are the plain call's"""
    from pyfeaturetrack_amd.backend import Context, context_of
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    c = block_case()
    fresh = Context(0)
    try:
        _load(fresh, c)
        fin, _ = fresh.select(10, c["n"], use_pyramid=True)
        fresh.track(10, 11, fin)
        assert fresh.motion_check_path() == 0
        old = _quiet()
        try:
            tc = _tc(c)
            path = context_of(tc).motion_check_path()
            fl = KLTSelectGoodFeatures(tc, c["frames"][0], c["n"])
            fwd, _ = fresh.track(10, 11, _records(fl))
            KLTTrackFeatures(tc, c["frames"][0], c["frames"][1], fl)
            assert context_of(tc).motion_check_path() == path and not hasattr(tc, "model_last")
            got = _records(fl)
            assert np.array_equal(got["x"], fwd["x"]) and np.array_equal(got["y"], fwd["y"]) and np.array_equal(got["val"], fwd["val"])
            assert not (got["val"] == KLT_MODEL_OUTLIER).any()
        finally:
            _restore(old)
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ Python API
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


def _summary_equals(summary, want_model):
    A, t = model_affine(want_model) if want_model["valid"] else (None, None)
    assert (summary["valid"], summary["candidates"], summary["inliers"], summary["hypothesis"]) == (
        want_model["valid"], want_model["n_candidates"], want_model["n_inliers"], want_model["hypothesis"]), (summary, want_model)
    if A is None:
        assert summary["A"] is None and summary["t"] is None
    else:
        assert np.array_equal(summary["A"], A) and np.array_equal(summary["t"], t)


@pytest.mark.parametrize("sequential", [False, True], ids=["pingpong", "sequential"])
@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fb"])
def test_track_features_runs_the_check(ctx, sequential, fb):
    """KLTTrackFeatures with tc.motionModelCheck over three steps of the moving-block clip, lost features replaced after every step: the
    list it leaves is the plain (or forward-backward) tracker call on the records it held, then the rule; tc.model_last is the rule's model"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    c = block_case()
    ncols, nrows = c["size"]
    frames, n = c["frames"], c["n"]
    old = _quiet()
    _load(ctx, c)
    try:
        tc = _tc(c, sequentialMode=sequential, motionModelCheck="affine", model_seed=11, forwardBackwardCheck=fb, trackQuality=True)
        kw = dict(hypotheses=256, seed=11, min_inliers=8, max_error=1.0, min_area=1.0)
        fl = KLTSelectGoodFeatures(tc, frames[0], n)
        flagged = 0
        for k in range(1, 4):
            before = _records(fl)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            after = _records(fl)
            fwd = (ctx.track_fb if fb else ctx.track)(10 + k - 1, 10 + k, before)[0]
            want_out, want_model = motion_check_expected(before, fwd, ncols, nrows, **kw)
            live = before["val"] >= 0
            _same_xyv(after[live], want_out[live], "step %d" % k)
            _summary_equals(tc.model_last, want_model)
            assert want_model["valid"] == 1
            flag = want_out["val"] == KLT_MODEL_OUTLIER
            assert (tc.quality_last["val"][flag] == 0).all()                    # the quality launch runs behind the check
            assert (tc.quality_last["val"][live & (want_out["val"] == KLT_TRACKED)] == 1).sum() >= 50
            flagged += int(flag.sum())
            KLTReplaceLostFeatures(tc, frames[k], fl)
        assert flagged >= 10, flagged
    finally:
        _restore(old)
        _free(ctx, c)


@pytest.mark.parametrize("prefetch", [True, False])
def test_track_sequence_carries_the_models(ctx, prefetch):
    """KLTTrackSequence with tc.motionModelCheck, 6 frames, lost features replaced: row k of the table is the plain tracker call on row k - 1,
    then the rule, then the replacement pass, which refills flagged slots; ft.models[k] is the rule's model, row 0 all zero"""
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    c = block_case()
    ncols, nrows = c["size"]
    frames, n = c["frames"], c["n"]
    old = _quiet()
    try:
        tc = _tc(c)
        plain = KLTTrackSequence(tc, frames, n, prefetch=prefetch)
        assert plain.models is None and not (plain.rec["val"] == KLT_MODEL_OUTLIER).any()
        tc.motionModelCheck = "affine"
        ft = KLTTrackSequence(tc, frames, n, prefetch=prefetch)
        assert ft.models.shape == (len(frames),) and ft.models.dtype == MODEL_DTYPE
        assert ft.models[0].tobytes() == np.zeros((), MODEL_DTYPE).tobytes()
        assert np.array_equal(ft.rec[0], plain.rec[0])
        _load(ctx, c)
        kw = dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0, min_area=1.0)
        flagged = refilled = 0
        for k in range(1, len(frames)):
            before, after = np.ascontiguousarray(ft.rec[k - 1]), np.ascontiguousarray(ft.rec[k])
            fwd, _ = ctx.track(10 + k - 1, 10 + k, before)
            want_out, want_model = motion_check_expected(before, fwd, ncols, nrows, **kw)
            assert ft.models[k].tobytes() == want_model.tobytes(), (k, ft.models[k], want_model)
            kept = after["val"] <= 0                                 # not refilled by frame k's replacement pass
            _same_xyv(after[kept], want_out[kept], "row %d" % k)
            flag = want_out["val"] == KLT_MODEL_OUTLIER
            flagged += int(flag.sum())
            refilled += int((flag & (after["val"] > 0)).sum())
            assert (want_out["val"][after["val"] > 0] < 0).all()     # only lost slots are refilled
        print("flagged %d over the clip, %d of them refilled on the same frame's replacement pass" % (flagged, refilled))
        assert flagged >= 10 and refilled >= 5, (flagged, refilled)
    finally:
        _restore(old)
        _free(ctx, c)
