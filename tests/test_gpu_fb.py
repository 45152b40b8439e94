"""The fused forward-backward check (klt_track_fb*) against the composition it stands for: two plain tracker runs and the rule of
tests/fb_expected.py.  Every comparison is exact -- x, y, val, aux of `out` and of `back`; a difference is a bug, not a tolerance."""
import numpy as np
import pytest

from fb_expected import KLT_FB_INCONSISTENT, KLT_TRACKED, OCCLUSION_CASES, fb_compose, occlusion_pair
from helpers import baseline_case, make_tc, params_from_tc, synth251_frames

pytestmark = pytest.mark.gpu

OPT_TRACK_VARIANT, OPT_XCD_ORDER, OPT_TREE_SUMS, OPT_FAIL_ALLOC_AFTER = 11, 13, 18, 19


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_records(got, want, what):
    for name in ("val", "x", "y", "aux"):
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, "%s.%s: %d of %d differ, first at %d: got %r, want %r (records %r / %r)" % (
            what, name, bad.size, len(got), bad[0], got[name][bad[0]], want[name][bad[0]], got[bad[0]], want[bad[0]])


def load_pair(ctx, tc, f0, f1, n, lost_every=0):
    """both frames in slots 0 / 1 with pyramids, n features selected on frame 0 (some marked lost if asked)"""
    ctx.configure(tc)
    ctx.upload(0, f0)
    ctx.upload(1, f1)
    ctx.build_pyramids(0)
    ctx.build_pyramids(1)
    fl, _ = ctx.select(0, n)
    if lost_every:
        fl["val"][3::lost_every] = -3
    return fl


def gpu_tracker(ctx):
    def track(fl, a, b):
        return ctx.track(a - 1, b - 1, fl)[0]
    return track


def check_fused(ctx, fl, max_error, what, need_rejected=False):
    """klt_track_fb on `fl` (slots 0 -> 1) against two klt_track calls and the rule; returns (out, back, fwd)"""
    ctx.set_fb_params(max_error=max_error)
    want, fwd, back = fb_compose(gpu_tracker(ctx), fl, max_error)
    out, k, got_back = ctx.track_fb(0, 1, fl, want_back=True)
    assert_records(out, want, what + " out")
    assert_records(got_back, back, what + " back")
    assert k == int((out["val"] >= 0).sum())
    out2, _ = ctx.track_fb(0, 1, fl)                                  # without the backward records: the same `out`
    assert_records(out2, want, what + " out (no back)")
    rejected = out["val"] == KLT_FB_INCONSISTENT
    print("%s: %d live, %d tracked forward, %d rejected" % (what, int((fl["val"] >= 0).sum()),
                                                            int(((fl["val"] >= 0) & (fwd["val"] == KLT_TRACKED)).sum()), int(rejected.sum())))
    if need_rejected:
        assert rejected.any() and (out["val"] == KLT_TRACKED).any(), what
    return out, got_back, fwd


def test_cfg1_and_synth251(ctx, img0, img1):
    fl = load_pair(ctx, make_tc(max_residue=10.0), img0, img1, 100)
    check_fused(ctx, fl, 1.0, "cfg-1")
    frames = synth251_frames()
    fl = load_pair(ctx, make_tc(), frames[0], frames[2], 80, lost_every=9)
    check_fused(ctx, fl, 1.0, "synth251")


@pytest.mark.parametrize("case", OCCLUSION_CASES, ids=[c[0] for c in OCCLUSION_CASES])
@pytest.mark.parametrize("max_error", [0.0, 0.05, 1.0, 1e9])
def test_occlusion_cases_and_thresholds(ctx, case, max_error):
    name, width, height, window, levels, ss, block, n = case
    f0, f1 = occlusion_pair(width, height, block)
    fl = load_pair(ctx, make_tc(levels=levels, ss=ss, window=window), f0, f1, n, lost_every=13)
    out, back, fwd = check_fused(ctx, fl, max_error, "%s, max_error %g" % (name, max_error), need_rejected=max_error == 1.0)
    checked = (fl["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
    if max_error == 1e9:                           # nothing exceeds the limit: only features the backward run lost are rejected
        assert np.array_equal(out["val"] == KLT_FB_INCONSISTENT, checked & (back["val"] != KLT_TRACKED))
    if max_error == 0.0:                           # only a round trip that ends exactly where it started is kept
        kept = checked & (out["val"] == KLT_TRACKED)
        assert np.array_equal(kept, checked & (back["val"] == KLT_TRACKED) & (back["x"] == fl["x"]) & (back["y"] == fl["y"]))


@pytest.mark.parametrize("window,levels,ss", [(5, 2, 4), (13, 2, 2), (21, 2, 2), (31, 1, 2)])
def test_any_window_kernels(ctx, window, levels, ss):
    """the forward-backward forms of the any-window kernel with 1, 4, 8 and 16 samples per lane (windows 7, 9 and 15 are the cases
    above).  With max_error = 1.0 the CPU oracle's composition rejects 17, 17, 8 and 2 of the 123, 127, 112 and 106 features it tracks
    forward (of 138 live ones).  Window 13 also as a batch of two pairs: the batched form of the same kernel"""
    f0, f1 = occlusion_pair(320, 240, (70, 170, 100, 220))
    fl = load_pair(ctx, make_tc(levels=levels, ss=ss, window=window), f0, f1, 150, lost_every=13)
    out, back, _ = check_fused(ctx, fl, 1.0, "window %d" % window, need_rejected=True)
    if window == 13:
        ctx.featbuf_upload(100, fl)
        ctx.track_fb_batch_async([(0, 1, 100, 200 + i, 300 + i) for i in range(2)], len(fl))
        ctx.sync()
        for i in range(2):
            assert_records(ctx.featbuf_download(200 + i, len(fl)), out, "window 13, batch pair %d out" % i)
            assert_records(ctx.featbuf_download(300 + i, len(fl)), back, "window 13, batch pair %d back" % i)


@pytest.mark.parametrize("case", OCCLUSION_CASES + [("cfg-1",)], ids=[c[0] for c in OCCLUSION_CASES] + ["cfg1"])
def test_against_the_cpu_oracle_composition(ctx, case, img0, img1):
    """the fused kernel against two runs of the CPU oracle's tracker and the rule (the oracle writes no aux word: x, y, val)"""
    from oracle import klt_oracle as ko
    from test_fb_rule import oracle_tracker
    if case[0] == "cfg-1":
        f0, f1, tc, n = img0, img1, make_tc(max_residue=10.0), 100
    else:
        name, width, height, window, levels, ss, block, n = case
        f0, f1 = occlusion_pair(width, height, block)
        tc = make_tc(levels=levels, ss=ss, window=window)
    fl = load_pair(ctx, tc, f0, f1, n)
    p = params_from_tc(tc)
    ofl = ko.select_good_features(p, f0.astype(np.float32), n)
    for name in ("x", "y", "val"):
        assert np.array_equal(fl[name], ofl[name])
    want, _, oback = fb_compose(oracle_tracker(ko, p, f0, f1), ofl, 1.0)
    ctx.set_fb_params(max_error=1.0)
    out, _, back = ctx.track_fb(0, 1, fl, want_back=True)
    for name in ("val", "x", "y"):
        assert np.array_equal(out[name], want[name]), (case[0], name)
        assert np.array_equal(back[name], oback[name]), (case[0], "back", name)


@pytest.mark.parametrize("tag,n", [("cfg2", 5000), ("cfg2", 500), ("cfg3", 5000)])
def test_baseline_sizes(ctx, tag, n):
    """cfg-2 with 5000 features (7x7, four features per wavefront), with 500 (one feature per wavefront), cfg-3 (15x15 quad kernel);
    an occluded block in frame 1 so that the check has something to reject"""
    frames, tc, _ = baseline_case(tag)
    f1 = frames[1].copy()
    f1[300:700, 600:1300] = frames[0][100:500, 200:900]
    fl = load_pair(ctx, tc, frames[0], f1, n, lost_every=17)
    check_fused(ctx, fl, 1.0, "%s, %d features" % (tag, n), need_rejected=True)


def test_kernel_options(ctx):
    """KLT_OPT_TRACK_VARIANT 0 (window 9, 7 and 15 on the plain kernel), KLT_OPT_TRACK_XCD_ORDER 0 / 1, and KLT_OPT_TRACK_TREE_SUMS, which
    the check does not look at: the composition is always that of two default-sum runs"""
    for window, levels, ss in ((9, 2, 2), (7, 3, 4), (15, 3, 2)):
        f0, f1 = occlusion_pair(640, 480, (140, 340, 200, 440))
        fl = load_pair(ctx, make_tc(levels=levels, ss=ss, window=window), f0, f1, 2400, lost_every=11)
        want, _, wback = fb_compose(gpu_tracker(ctx), fl, 1.0)
        ctx.set_fb_params(max_error=1.0)
        try:
            for variant in (0, 4):
                for order in (0, 1):
                    for tree in (0, 1):
                        ctx.set_option(OPT_TRACK_VARIANT, variant)
                        ctx.set_option(OPT_XCD_ORDER, order)
                        ctx.set_option(OPT_TREE_SUMS, tree)
                        out, _, back = ctx.track_fb(0, 1, fl, want_back=True)
                        what = "window %d, variant %d, order %d, tree %d" % (window, variant, order, tree)
                        assert_records(out, want, what)
                        assert_records(back, wback, what + " back")
        finally:
            ctx.set_option(OPT_TRACK_VARIANT, 4)
            ctx.set_option(OPT_XCD_ORDER, 1)
            ctx.set_option(OPT_TREE_SUMS, 0)


@pytest.mark.parametrize("attrs", [dict(retainTrackers=True), dict(max_residue=6.0), dict(max_residue=10.0, retainTrackers=True),
                                   dict(step_factor=0.8, min_determinant=0.5, min_displacement=0.03, max_iterations=7)],
                         ids=["retain", "max_residue", "retain+residue", "step_det_displacement"])
@pytest.mark.parametrize("n", [400, 2400])
def test_tracker_parameters(ctx, attrs, n):
    f0, f1 = occlusion_pair(640, 480, (140, 340, 200, 440))
    fl = load_pair(ctx, make_tc(levels=3, ss=4, **attrs), f0, f1, n, lost_every=7)
    check_fused(ctx, fl, 0.5, "%r, %d features" % (attrs, n))


def test_batch_of_eight_pairs(ctx):
    """klt_track_fb_batch_async on 8 pairs (some with an occluded block) = the per-pair calls; without fb_back the same `out`"""
    tc = make_tc(levels=3, ss=4)
    ctx.configure(tc)
    ctx.set_fb_params(max_error=1.0)
    n, npairs = 700, 8
    want, wback = [], []
    for i in range(npairs):
        if i % 2:
            f0, f1 = occlusion_pair(640, 480, (100 + 10 * i, 300, 150, 400 + 10 * i), seed=30 + i)
        else:
            from pyfeaturetrack_amd import synth
            f0, f1 = synth.synth_pair(640, 480, 30 + i, shift=(1.3, -0.8))
        ctx.upload(10 + 2 * i, f0)
        ctx.upload(11 + 2 * i, f1)
        ctx.build_pyramids(10 + 2 * i)
        ctx.build_pyramids(11 + 2 * i)
        fl, _ = ctx.select(10 + 2 * i, n)
        fl["val"][i::19] = -2
        ctx.featbuf_upload(100 + i, fl)
        o, _, b = ctx.track_fb(10 + 2 * i, 11 + 2 * i, fl, want_back=True)
        want.append(o)
        wback.append(b)
    assert any((o["val"] == KLT_FB_INCONSISTENT).any() for o in want)
    ctx.track_fb_batch_async([(10 + 2 * i, 11 + 2 * i, 100 + i, 200 + i, 300 + i) for i in range(npairs)], n)
    ctx.sync()
    for i in range(npairs):
        assert_records(ctx.featbuf_download(200 + i, n), want[i], "batch pair %d out" % i)
        assert_records(ctx.featbuf_download(300 + i, n), wback[i], "batch pair %d back" % i)
    ctx.track_fb_batch_async([(10 + 2 * i, 11 + 2 * i, 100 + i, 400 + i) for i in range(npairs)], n)
    ctx.sync()
    for i in range(npairs):
        assert_records(ctx.featbuf_download(400 + i, n), want[i], "batch pair %d out, no back" % i)
    # 8 x 700 features take the four-features-per-wavefront kernel (n * npairs >= 2048); two pairs stay on the one-feature kernel
    ctx.track_fb_batch_async([(10 + 2 * i, 11 + 2 * i, 100 + i, 500 + i, 600 + i) for i in range(2)], n)
    ctx.sync()
    for i in range(2):
        assert_records(ctx.featbuf_download(500 + i, n), want[i], "two-pair batch out %d" % i)
        assert_records(ctx.featbuf_download(600 + i, n), wback[i], "two-pair batch back %d" % i)
    for s in range(10, 10 + 2 * npairs):
        ctx.slot_free(s)


def test_error_paths(ctx, img0, img1):
    from pyfeaturetrack_amd._abi import KltBackendError, KltFbParams, KltOutOfMemory
    fl = load_pair(ctx, make_tc(), img0, img1, 60)
    ctx.featbuf_upload(100, fl)
    for bufs in ((100, 100, -1), (100, 101, 100), (100, 101, 101), (100, 101, -2)):
        with pytest.raises(KltBackendError, match="distinct|fb_back"):
            ctx.track_fb_async(0, 1, bufs[0], bufs[1], len(fl), bufs[2])
    with pytest.raises(KltBackendError, match="distinct"):
        ctx.track_fb_batch_async([(0, 1, 100, 101, 102), (0, 1, 100, 103, 100)], len(fl))
    for bad in (-1.0, float("nan")):
        with pytest.raises(KltBackendError, match="max_error"):
            ctx.set_fb_params(KltFbParams(1, bad))
    ctx.set_fb_params(max_error=1.0)
    ctx.upload(7, img0)                                              # a frame without pyramids
    with pytest.raises(KltBackendError, match="pyramids"):
        ctx.track_fb_async(0, 7, 100, 101, len(fl), -1)
    ctx.slot_free(7)
    # every allocation site of one klt_track_fb call refused in turn: KLT_ERR_NOMEM, and the context goes on working.  A fresh context
    # and a list longer than anything it has seen: the call has to allocate its record buffers and the feature order
    from pyfeaturetrack_amd.backend import Context
    want, _, wback = ctx.track_fb(0, 1, np.concatenate([fl, fl, fl]), want_back=True)
    c = Context(0)
    try:
        fl3 = np.concatenate([load_pair(c, make_tc(), img0, img1, 60)] * 3)
        c.set_fb_params(max_error=1.0)
        refused = 0
        for k in range(12):
            c.set_option(OPT_FAIL_ALLOC_AFTER, k)
            try:
                out, _, back = c.track_fb(0, 1, fl3, want_back=True)
            except KltOutOfMemory:
                refused += 1
                continue
            finally:
                c.set_option(OPT_FAIL_ALLOC_AFTER, -1)
            assert_records(out, want, "after %d refused allocations" % refused)
            assert_records(back, wback, "back after %d refused allocations" % refused)
            break
        else:
            raise AssertionError("the call never got through")
        print("allocations refused in turn: %d" % refused)
        assert refused >= 2
        out, _ = c.track_fb(0, 1, fl3)
        assert_records(out, want, "context after the walk")
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ Python API
def _quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    return old


def _records(fl):
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    a = np.zeros(len(fl), FEAT_DTYPE)
    a["x"], a["y"], a["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return a


def _api_tracker(make_plain, frames):
    """plain KLTTrackFeatures calls on fresh lists as the tracker of fb_compose (frames: {1: ..., 2: ...})"""
    from pyfeaturetrack_amd.klt import KLT_Feature
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures

    def track(rec, a, b):
        fl = [KLT_Feature() for _ in range(len(rec))]
        for f, r in zip(fl, rec):
            f.x, f.y, f.val = float(r["x"]), float(r["y"]), int(r["val"])
        KLTTrackFeatures(make_plain(), frames[a], frames[b], fl)
        return _records(fl)
    return track


def _assert_xyv(got, want, what):
    for name in ("val", "x", "y"):
        assert np.array_equal(got[name], want[name]), (what, name, np.flatnonzero(got[name] != want[name])[:5])


@pytest.mark.parametrize("pillow", [False, True], ids=["numpy", "pillow"])
def test_python_api_pair(pillow):
    from pyfeaturetrack_amd.klt import kltState
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        f0, f1 = occlusion_pair(320, 240, (70, 170, 100, 220))
        if pillow:
            PIL = pytest.importorskip("PIL.Image")
            f0, f1 = PIL.fromarray(f0, "L"), PIL.fromarray(f1, "L")
        tc = make_tc(forwardBackwardCheck=True, fb_max_error=0.75)
        fl = KLTSelectGoodFeatures(tc, f0, 150)
        fin = _records(fl)
        want, _, wback = fb_compose(_api_tracker(make_tc, {1: f0, 2: f1}), fin, 0.75)
        KLTTrackFeatures(tc, f0, f1, fl)
        got = _records(fl)
        _assert_xyv(got, want, "KLTTrackFeatures with the check")
        rejected = got["val"] == kltState.KLT_FB_INCONSISTENT
        assert rejected.any() and (got["x"][rejected] == -1.0).all() and (got["y"][rejected] == -1.0).all()
        _assert_xyv(np.asarray(tc.fb_back), wback, "tc.fb_back")
        # foreign feature objects take the per-object branch
        class Feat:
            pass
        objs = []
        for r in fin:
            o = Feat()
            o.x, o.y, o.val = float(r["x"]), float(r["y"]), int(r["val"])
            o.aff_img = o.aff_img_gradx = o.aff_img_grady = None
            objs.append(o)
        KLTTrackFeatures(tc, f0, f1, objs)
        _assert_xyv(_records(objs), want, "per-object branch")
    finally:
        from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
        sgf.KLT_verbose, tf.KLT_verbose = old


def test_python_api_sequential_and_edited_frame():
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd import synth
    old = _quiet()
    try:
        base = synth.synth_base(320, 240, 5)
        frames = [synth.synth_frame(320, 240, 5, k, shift=(1.3, -0.8), base=base) for k in range(3)]
        frames[1][60:140, 90:200] = synth.shift_frame(synth.synth_base(320, 240, 6), 0, 0)[60:140, 90:200]
        tc = make_tc(forwardBackwardCheck=True, sequentialMode=True)
        fl = KLTSelectGoodFeatures(tc, frames[0], 120)
        for k in (1, 2):                               # three frames in sequential mode
            fin = _records(fl)
            want = fb_compose(_api_tracker(make_tc, {1: frames[k - 1].copy(), 2: frames[k].copy()}), fin, 1.0)[0]
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            _assert_xyv(_records(fl), want, "sequential step %d" % k)
        assert (_records(fl)["val"] == KLT_FB_INCONSISTENT).any()
        # the same array edited in place off the lattice: taken as resident, found different, sent again, tracked again
        tc = make_tc(forwardBackwardCheck=True)
        f0, f1 = frames[0].copy(), frames[2].copy()
        fl = KLTSelectGoodFeatures(tc, f0, 120)
        KLTTrackFeatures(tc, f0, f1, fl)
        f1[61:139:2, 91:199:2] = 17                    # off the 1024-pixel lattice or not: every byte is compared
        f1[50:120, 30:100] = frames[1][50:120, 30:100]
        fl = KLTSelectGoodFeatures(tc, f0, 120)
        fin = _records(fl)
        want = fb_compose(_api_tracker(make_tc, {1: f0.copy(), 2: f1.copy()}), fin, 1.0)[0]
        KLTTrackFeatures(tc, f0, f1, fl)
        _assert_xyv(_records(fl), want, "edited frame")
    finally:
        from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
        sgf.KLT_verbose, tf.KLT_verbose = old


@pytest.mark.parametrize("prefetch", [True, False])
def test_sequence_with_the_check(prefetch):
    """KLTTrackSequence with the flag = the per-frame loop KLTTrackFeatures + KLTReplaceLostFeatures with the flag; and the flag matters"""
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, storeFeatures as sf, synth, trackFeatures as tf
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    old = _quiet()
    try:
        base = synth.synth_base(640, 480, 9)
        frames = [synth.synth_frame(640, 480, 9, k, shift=(1.3, -0.8), base=base) for k in range(5)]
        frames[2][100:260, 200:420] = synth.shift_frame(synth.synth_base(640, 480, 10), 0, 0)[100:260, 200:420]
        n = 300

        def make(flag=True):
            return make_tc(levels=3, ss=4, sequentialMode=True, forwardBackwardCheck=flag)
        tc = make()
        want = sf.KLTCreateFeatureTable(len(frames), n)
        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
        sf.KLTStoreFeatureList(fl, want, 0)
        rejected = 0
        for k in range(1, len(frames)):
            tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            rejected += int((_records(fl)["val"] == KLT_FB_INCONSISTENT).sum())
            sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
            sf.KLTStoreFeatureList(fl, want, k)
        assert rejected > 0
        got = KLTTrackSequence(make(), (f for f in frames), n, prefetch=prefetch)
        assert np.array_equal(got.val, want.val) and np.array_equal(got.x, want.x) and np.array_equal(got.y, want.y)
        plain = KLTTrackSequence(make(False), (f for f in frames), n, prefetch=prefetch)
        assert not (np.array_equal(plain.val, want.val) and np.array_equal(plain.x, want.x))
    finally:
        sgf.KLT_verbose, tf.KLT_verbose = old
