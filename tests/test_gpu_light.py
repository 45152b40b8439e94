"""Gain / bias tracking (klt_set_light_params mode 1) on the device against the numpy restatement of the rule
(tests/light_expected.py).  Every comparison is exact -- x, y, val and the aux iteration word; a difference is a bug in the kernels or in the
restatement's transcription of the rule, not a tolerance."""
import numpy as np
import pytest

from helpers import make_tc
from light_expected import (FEAT_DTYPE, KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS, KLT_OOB, KLT_SMALL_DET, KLT_TRACKED, level_iterations,
                            light_case, light_track, shares)

pytestmark = pytest.mark.gpu

OPT_TRACK_VARIANT = 11
FB_IN, FB_OUT, FB_BACK, FB_GUESS = 100, 102, 103, 101


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_records(got, want, what, fields=("val", "x", "y", "aux")):
    for name in fields:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, "%s.%s: %d of %d differ, first at %d: got %r, want %r (records %r / %r)" % (
            what, name, bad.size, len(got), bad[0], got[name][bad[0]], want[name][bad[0]], got[bad[0]], want[bad[0]])


def load(ctx, c, s0=0, s1=1, mode=1):
    ctx.configure(c["tc"])                       # (a tracking context without the switch: mode 0)
    ctx.upload(s0, c["f1"])
    ctx.upload(s1, c["f2"])
    ctx.build_pyramids(s0)
    ctx.build_pyramids(s1)
    ctx.set_light_params(mode=mode)


WAVE_CASES = [
    ("w7", dict(window=7)),
    ("w7_residue", dict(window=7, max_residue=10.0)),
    ("w15", dict(window=15)),
    ("w15_residue", dict(window=15, max_residue=10.0)),
    ("w5_maxk1_residue", dict(window=5, max_residue=10.0)),
    ("w9_maxk2", dict(window=9)),
    ("w17_maxk8_residue", dict(window=17, max_residue=10.0)),
    ("w7_retain_residue", dict(window=7, max_residue=10.0, retainTrackers=True)),
    ("w7_step_det_displacement", dict(window=7, step_factor=0.8, min_determinant=0.5, min_displacement=0.03)),
    ("w7_three_levels_320x240", dict(width=320, height=240, window=7, levels=3, ss=4, edge=False, borderx=8, bordery=8, max_residue=10.0)),
]


@pytest.mark.parametrize("name,kw", WAVE_CASES, ids=[c[0] for c in WAVE_CASES])
def test_wave_kernel_equals_the_rule(ctx, name, kw):
    """300 features, one per wavefront: compile-time windows 7 and 15, run-time windows 5, 9 and 17, the residue test on and off,
    retainTrackers, other step / determinant / displacement parameters, three levels.  The lists reach every image edge (templates off
    the image, windows that leave it in the Newton loop and after it), the iteration cap and the zeroed rectangle of frame 2."""
    c = light_case(**kw)
    fin, want = c["fin"], c["want"]
    live = fin["val"] >= 0
    if kw.get("edge", True):                    # what the list is there for, read off the rule's records
        lost_at = {v: int((want["val"][live] == v).sum()) for v in (KLT_TRACKED, KLT_OOB, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_LARGE_RESIDUE)}
        print(name, lost_at)
        assert lost_at[KLT_TRACKED] >= 10 and lost_at[KLT_OOB] >= 50
        its = [level_iterations(want["aux"][live], r) for r in (0, 1)]
        assert (its[1] == 0).any()                                               # a template off the image, or a window off it at once
        assert ((want["val"][live] == KLT_OOB) & (its[0] > 0)).any()             # a window that left the image after some iterations
        assert (its[0] == c["tc"].max_iterations).any()                          # the iteration cap
        if not c["tc"].retainTrackers:
            assert lost_at[KLT_SMALL_DET] >= 10                                  # the zeroed rectangle
            if c["tc"].max_residue is not None:
                assert lost_at[KLT_LARGE_RESIDUE] >= 1
    else:
        assert (level_iterations(want["aux"][live], 0) >= 0).sum() >= 50         # features that came down all three levels
    load(ctx, c)
    got, _ = ctx.track(0, 1, fin)
    assert ctx.track_light_path() == 1
    assert_records(got, want, name)


def test_quad_kernel_equals_the_rule_and_the_wave_kernel(ctx):
    """2051 features (7x7; not a multiple of four: the last wavefront has idle lane groups) take the four-features-per-wavefront kernel;
    with KLT_OPT_TRACK_VARIANT 0 the same list takes the wave kernel and gives the same records"""
    c = light_case(n=2051, max_residue=10.0)
    fin, want = c["fin"], c["want"]
    load(ctx, c)
    try:
        got, _ = ctx.track(0, 1, fin)
        assert ctx.track_light_path() == 2
        assert_records(got, want, "quad kernel")
        ctx.set_option(OPT_TRACK_VARIANT, 0)
        wave, _ = ctx.track(0, 1, fin)
        assert ctx.track_light_path() == 1
        assert_records(wave, want, "wave kernel, variant 0")
        assert_records(wave, got, "wave against quad")
    finally:
        ctx.set_option(OPT_TRACK_VARIANT, 4)
    c = light_case(n=2051)                      # ... and without the residue test
    load(ctx, c)
    got, _ = ctx.track(0, 1, c["fin"])
    assert ctx.track_light_path() == 2
    assert_records(got, c["want"], "quad kernel, no residue test")


@pytest.mark.parametrize("n,path", [(1030, 2), (200, 1)], ids=["quad", "wave"])
def test_batched_pairs_equal_their_single_calls(ctx, n, path):
    """two pairs in one launch: 2 x 1030 features reach the quad kernel, 2 x 200 the wave kernel; each pair's records are its single-pair
    call's and the rule's"""
    a = light_case(n=n, max_residue=10.0)
    b = light_case(n=n, max_residue=10.0, list_seed=9)
    load(ctx, a, 0, 1)
    ctx.upload(2, a["f2"])                      # the second pair: the frames the other way round, another list
    ctx.upload(3, a["f1"])
    ctx.build_pyramids(2)
    ctx.build_pyramids(3)
    want_b = light_track(a["p"], a["pyr2"], a["pyr1"], b["fin"])
    single_a, _ = ctx.track(0, 1, a["fin"])
    single_b, _ = ctx.track(2, 3, b["fin"])
    ctx.featbuf_upload(300, a["fin"])
    ctx.featbuf_upload(301, b["fin"])
    ctx.track_batch_async([(0, 1, 300, 310), (2, 3, 301, 311)], n)
    ctx.sync()
    assert ctx.track_light_path() == path
    got_a, got_b = ctx.featbuf_download(310, n), ctx.featbuf_download(311, n)
    assert_records(got_a, single_a, "pair 0 against its single call")
    assert_records(got_b, single_b, "pair 1 against its single call")
    assert_records(got_a, a["want"], "pair 0 against the rule")
    assert_records(got_b, want_b, "pair 1 against the rule")
    ctx.slot_free(2)
    ctx.slot_free(3)


def test_mode_off_is_the_plain_tracker(ctx):
    """mode 1 -> 0: the records are the plain tracker's (the CPU oracle's) bit for bit, and klt_track_light_path keeps its value"""
    from oracle import klt_oracle as ko
    c = light_case(n=300, max_residue=10.0)
    load(ctx, c)
    lit, _ = ctx.track(0, 1, c["fin"])
    assert_records(lit, c["want"], "mode 1")
    path = ctx.track_light_path()
    assert path == 1
    ctx.set_light_params(mode=0)
    got, _ = ctx.track(0, 1, c["fin"])
    plain = c["fin"].copy()
    ko.track_features(c["p"], c["pyr1"], c["pyr2"], plain)
    assert_records(got, plain, "mode 0", ("val", "x", "y"))
    assert ctx.track_light_path() == path
    assert (got["val"] != lit["val"]).any()
    ctx.featbuf_upload(FB_IN, c["fin"])          # ... nor does a batched or an asynchronous plain launch touch it
    ctx.track_async(0, 1, FB_IN, FB_OUT, len(c["fin"]))
    ctx.track_batch_async([(0, 1, FB_IN, FB_OUT)], len(c["fin"]))
    ctx.sync()
    assert ctx.track_light_path() == path
    assert_records(ctx.featbuf_download(FB_OUT, len(c["fin"])), plain, "mode 0, batched", ("val", "x", "y"))


def test_other_entry_points_are_refused(ctx):
    """with mode 1 the forward-backward, motion-prior and affine entry points return KLT_ERR_STATE; the context tracks on afterwards"""
    from pyfeaturetrack_amd._abi import KltBackendError, KltLightParams
    c = light_case(n=300, max_residue=10.0)
    fin, n = c["fin"], len(c["fin"])
    load(ctx, c)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, fin)
    ctx.set_fb_params(max_error=1.0)
    ctx.affine_alloc(0, n)
    calls = [
        lambda: ctx.track_fb_async(0, 1, FB_IN, FB_OUT, n, FB_BACK),
        lambda: ctx.track_fb(0, 1, fin),
        lambda: ctx.track_fb_batch_async([(0, 1, FB_IN, FB_OUT)], n),
        lambda: ctx.track_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n),
        lambda: ctx.track_guess(0, 1, fin, fin),
        lambda: ctx.track_guess_batch_async([(0, 1, FB_IN, FB_GUESS, FB_OUT)], n),
        lambda: ctx.track_fb_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n, FB_BACK),
        lambda: ctx.track_affine_async(0, 1, FB_IN, FB_OUT, n, 0),
        lambda: ctx.track_affine(0, 1, fin, 0),
    ]
    try:
        for call in calls:
            with pytest.raises(KltBackendError, match=r"error -3: .*lighting compensation"):
                call()
        with pytest.raises(KltBackendError, match="mode must be"):
            ctx.set_light_params(KltLightParams(2))
        got, _ = ctx.track(0, 1, fin)
        assert_records(got, c["want"], "the context after the refused calls")
        ctx.set_light_params(mode=0)
        out, _, back = ctx.track_fb(0, 1, fin, want_back=True)          # ... and every one of them works again with mode 0
        assert len(out) == n and len(back) == n
    finally:
        ctx.affine_free(0)


# ------------------------------------------------------------------------------------------------ Python API
def _quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    return old


def _restore(old):
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    from pyfeaturetrack_amd.backend import default_context
    sgf.KLT_verbose, tf.KLT_verbose = old
    default_context().set_light_params(mode=0)      # the thread's shared context: whoever drives it directly next finds the plain tracker


def _records(fl):
    a = np.zeros(len(fl), FEAT_DTYPE)
    a["x"], a["y"], a["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return a


XYV = ("val", "x", "y")


def test_python_api_ping_pong_on_the_lit_pair(ctx):
    """KLTTrackFeatures with tc.lightingCompensation = "gain_bias" on numpy frames: the C ABI's records and the rule's; on the lit pair
    it keeps exactly what tests/test_light_rule.py measured on the CPU (230 of 300), the same call without the switch what the plain
    tracker keeps there (12)"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        c = light_case(320, 240, 7, 2, 4, n=300, edge=False, max_residue=10.0)
        tc = make_tc(levels=2, ss=4, window=7, max_residue=10.0, lightingCompensation="gain_bias")
        fl = KLTSelectGoodFeatures(tc, c["f1"], 300)
        fin = _records(fl)
        assert_records(fin, c["fin"], "the selection is the oracle's", XYV)
        KLTTrackFeatures(tc, c["f1"], c["f2"], fl)
        got = _records(fl)
        assert_records(got, c["want"], "KLTTrackFeatures against the rule", XYV)
        load(ctx, c)
        abi, _ = ctx.track(0, 1, fin)
        assert_records(got, abi, "KLTTrackFeatures against klt_track", XYV)
        assert shares(fin, got) == shares(c["fin"], c["want"]) == (230, 300)
        KLTTrackFeatures(tc, c["f1"], c["f2"], fl)              # the same pair again (both frames resident): the lost slots pass through
        again = light_track(c["p"], c["pyr1"], c["pyr2"], got)
        assert_records(_records(fl), again, "second call", XYV)
        plain_tc = make_tc(levels=2, ss=4, window=7, max_residue=10.0)
        fl = KLTSelectGoodFeatures(plain_tc, c["f1"], 300)
        KLTTrackFeatures(plain_tc, c["f1"], c["f2"], fl)
        plain = c["fin"].copy()
        ko.track_features(c["p"], c["pyr1"], c["pyr2"], plain)
        assert_records(_records(fl), plain, "without the switch: the plain tracker", XYV)
        assert shares(c["fin"], plain)[0] == 12
    finally:
        _restore(old)


def test_python_api_sequential_mode():
    """sequential mode: frame 2's pyramids become frame 1 of the next call; every step is the rule's"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        c = light_case(320, 240, 7, 2, 4, n=300, edge=False, max_residue=10.0)
        frames = [c["f1"], c["f2"], c["f1"]]
        pyr = [c["pyr1"], c["pyr2"], c["pyr1"]]
        tc = make_tc(levels=2, ss=4, window=7, max_residue=10.0, lightingCompensation="gain_bias", sequentialMode=True)
        fl = KLTSelectGoodFeatures(tc, frames[0], 300)
        for k in (1, 2):
            fin = _records(fl)
            want = light_track(c["p"], pyr[k - 1], pyr[k], fin)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            assert_records(_records(fl), want, "sequential step %d" % k, XYV)
            assert (want["val"] == KLT_TRACKED).sum() > 100
    finally:
        _restore(old)
