"""The motion prior (klt_track_guess*, klt_track_fb_guess_async, klt_predict_cv_async) against what it stands for: the plain tracker where
no guess counts, and the composition of tests/guess_expected.py from the CPU oracle's per-level step where one does.  Every comparison is
exact -- x, y, val and the aux word; a difference is a bug, not a tolerance."""
import functools

import numpy as np
import pytest

from fb_expected import OCCLUSION_CASES, occlusion_pair
from guess_expected import (FEAT_DTYPE, KLT_OOB, KLT_TRACKED, LARGE_SHIFT_CASES, fb_guess_compose, guess_compose,
                            large_shift_pair, noisy_truth, predict_cv)
from helpers import make_tc, params_from_tc

pytestmark = pytest.mark.gpu

OPT_TRACK_VARIANT, OPT_XCD_ORDER, OPT_TREE_SUMS, OPT_FAIL_ALLOC_AFTER = 11, 13, 18, 19
FB_IN, FB_GUESS, FB_OUT, FB_BACK = 100, 101, 102, 103
QUAD_PAIRS = 14                  # a 7x7 list takes the four-features-per-wavefront kernel from 2048 features per launch: 14 pairs of 149 / 150

PARAMETER_SETS = [dict(), dict(max_residue=10.0), dict(step_factor=0.8, min_determinant=0.5, min_displacement=0.03)]


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


@functools.lru_cache(maxsize=None)
def shift_case(index, attrs_index=0, n=None, mindist=None):
    """(tc, params, frames, oracle pyramids, selected list with a few lost slots, noisy-truth guesses, composition) of a large-shift case,
    computed once and shared"""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, shift, n_case = LARGE_SHIFT_CASES[index]
    attrs = dict(PARAMETER_SETS[attrs_index])
    if mindist is not None:
        attrs["mindist"] = mindist
    tc = make_tc(levels=levels, ss=ss, window=window, **attrs)
    p = params_from_tc(tc)
    f0, f1 = large_shift_pair(width, height, shift)
    fin = ko.select_good_features(p, f0.astype(np.float32), n or n_case)
    fin["val"][5::17] = -3
    pyr1, pyr2 = ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))
    guess, _ = noisy_truth(fin, shift)
    want = guess_compose(ko, p, pyr1, pyr2, fin, guess)
    for a in (fin, guess, want):
        a.setflags(write=False)
    return dict(name=name, tc=tc, p=p, f0=f0, f1=f1, fin=fin, pyr1=pyr1, pyr2=pyr2, guess=guess, want=want, shift=shift)


def load_frames(ctx, tc, f0, f1, s0=0, s1=1):
    ctx.configure(tc)
    ctx.upload(s0, f0)
    ctx.upload(s1, f1)
    ctx.build_pyramids(s0)
    ctx.build_pyramids(s1)


def run_guess(ctx, fin, guess, fb_guess=FB_GUESS):
    """one klt_track_guess_async launch on slots 0 -> 1; `guess` None: the list is its own guess list (fb_guess = fb_in)"""
    n = len(fin)
    ctx.featbuf_upload(FB_IN, fin)
    if guess is None:
        fb_guess = FB_IN
    else:
        ctx.featbuf_upload(fb_guess, guess)
    ctx.track_guess_async(0, 1, FB_IN, fb_guess, FB_OUT, n)
    ctx.sync()
    return ctx.featbuf_download(FB_OUT, n)


def run_guess_batch(ctx, fin, guess, npairs=QUAD_PAIRS):
    """the same pair `npairs` times in one batched launch (one output list each): every pair's records"""
    n = len(fin)
    ctx.featbuf_upload(FB_IN, fin)
    if guess is not None:
        ctx.featbuf_upload(FB_GUESS, guess)
    ctx.track_guess_batch_async([(0, 1, FB_IN, FB_IN if guess is None else FB_GUESS, 200 + i) for i in range(npairs)], n)
    ctx.sync()
    return [ctx.featbuf_download(200 + i, n) for i in range(npairs)]


def no_guess(fin):
    g = np.zeros(len(fin), FEAT_DTYPE)
    g["x"], g["y"] = fin["x"] + 20.0, fin["y"] - 20.0            # positions that would matter if they counted
    g["val"] = -1
    return g


@pytest.mark.parametrize("index", range(len(LARGE_SHIFT_CASES)), ids=[c[0] for c in LARGE_SHIFT_CASES])
@pytest.mark.parametrize("attrs_index", range(len(PARAMETER_SETS)), ids=["defaults", "max_residue", "step_det_displacement"])
def test_exactness_two_ways(ctx, index, attrs_index):
    """identity / invalid guesses = klt_track_async, noisy-truth guesses = the oracle composition; window 7 (one feature per wavefront in a
    single launch, four per wavefront in a 14-pair launch; 149 features: a short last group), 15 (quad kernel) and 9 (one sample per lane),
    KLT_OPT_TRACK_VARIANT 0 / 4 and KLT_OPT_TRACK_XCD_ORDER 0 / 1"""
    c = shift_case(index, attrs_index)
    fin, guess, want = c["fin"], c["guess"], c["want"]
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    window = c["tc"].window_width
    try:
        for variant in (0, 4):
            for order in (0, 1):
                ctx.set_option(OPT_TRACK_VARIANT, variant)
                ctx.set_option(OPT_XCD_ORDER, order)
                what = "%s, set %d, variant %d, order %d" % (c["name"], attrs_index, variant, order)
                plain, _ = ctx.track(0, 1, fin)
                assert_records(run_guess(ctx, fin, None), plain, what + ": identity guess")
                assert_records(run_guess(ctx, fin, no_guess(fin)), plain, what + ": invalid guesses")
                assert_records(run_guess(ctx, fin, guess), want, what + ": noisy truth")
                if window == 7:
                    for i, got in enumerate(run_guess_batch(ctx, fin, None)):
                        assert_records(got, plain, what + ": identity guess, batch pair %d" % i)
                    for i, got in enumerate(run_guess_batch(ctx, fin, guess)):
                        assert_records(got, want, what + ": noisy truth, batch pair %d" % i)
    finally:
        ctx.set_option(OPT_TRACK_VARIANT, 4)
        ctx.set_option(OPT_XCD_ORDER, 1)
    live = fin["val"] >= 0
    print("%s: %d live, %d tracked with the prior" % (c["name"], live.sum(), (want["val"][live] == KLT_TRACKED).sum()))
    assert (want["val"][live] == KLT_TRACKED).sum() > live.sum() // 3


@pytest.mark.parametrize("index", [0, 2], ids=["w7", "w15"])
def test_tree_sums_identity_guess(ctx, index):
    """KLT_OPT_TRACK_TREE_SUMS = 1: the identity guess gives klt_track_async's records under the same option (quad kernels: 7x7 in the
    14-pair launch, 15x15 in a single one)"""
    c = shift_case(index)
    fin = c["fin"]
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    ctx.set_option(OPT_TREE_SUMS, 1)
    try:
        if index == 0:
            ctx.featbuf_upload(FB_IN, fin)
            ctx.track_batch_async([(0, 1, FB_IN, 300 + i) for i in range(QUAD_PAIRS)], len(fin))
            ctx.sync()
            plain = ctx.featbuf_download(300, len(fin))
            for i, got in enumerate(run_guess_batch(ctx, fin, None)):
                assert_records(got, plain, "tree sums, 7x7, batch pair %d" % i)
        else:
            plain, _ = ctx.track(0, 1, fin)
            assert_records(run_guess(ctx, fin, None), plain, "tree sums, 15x15")
    finally:
        ctx.set_option(OPT_TREE_SUMS, 0)


def test_dense_list_takes_the_quad_kernels_in_a_single_launch(ctx):
    """2049 features on 320x240 (mindist 3): a single 7x7 launch takes the four-features-per-wavefront kernel, plain and forward-backward"""
    from oracle import klt_oracle as ko
    c = shift_case(0, 0, 2049, 3)
    fin, guess = c["fin"], c["guess"]
    assert (fin["val"] >= 0).sum() > 1500
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    plain, _ = ctx.track(0, 1, fin)
    assert_records(run_guess(ctx, fin, None), plain, "dense: identity guess")
    assert_records(run_guess(ctx, fin, guess), c["want"], "dense: noisy truth")
    want, _, wback = fb_guess_compose(ko, c["p"], c["pyr1"], c["pyr2"], fin, guess, 1.0)
    ctx.set_fb_params(max_error=1.0)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, guess)
    ctx.track_fb_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, len(fin), FB_BACK)
    ctx.sync()
    assert_records(ctx.featbuf_download(FB_OUT, len(fin)), want, "dense: forward-backward out")
    assert_records(ctx.featbuf_download(FB_BACK, len(fin)), wback, "dense: forward-backward back")


def mixed_guesses(fin, guess, width, height):
    """valid guesses mixed with every kind that does not count and every kind that is off the image"""
    g = guess.copy()
    kinds = [("val", -1), ("x", np.nan), ("y", np.nan), ("x", np.inf), ("y", -np.inf), ("x", 1e30), ("y", -1e30), ("x", -3.5), ("y", -0.25),
             ("x", width + 0.5), ("y", height + 2.0), ("x", width - 1.0), ("y", height - 0.5)]
    for k, (field, value) in enumerate(kinds):
        g[field][k::len(kinds) + 4] = value                     # (four of every seventeen stay valid guesses)
    return g


@pytest.mark.parametrize("index", range(len(LARGE_SHIFT_CASES)), ids=[c[0] for c in LARGE_SHIFT_CASES])
def test_mixed_guess_list_in_one_launch(ctx, index):
    """valid guesses, val < 0, NaN, +-inf, 1e30, negative values and positions just outside the image in one list: the records are the
    composition's -- a guess that does not count falls back to the feature's own position, one off the image gives KLT_OOB --, and the context
    works afterwards"""
    from oracle import klt_oracle as ko
    c = shift_case(index)
    fin = c["fin"]
    width, height = c["f0"].shape[1], c["f0"].shape[0]
    g = mixed_guesses(fin, c["guess"], width, height)
    want = guess_compose(ko, c["p"], c["pyr1"], c["pyr2"], fin, g)
    live = fin["val"] >= 0
    off = live & (g["val"] >= 0) & np.isfinite(g["x"]) & np.isfinite(g["y"]) & (
        (g["x"] < 0) | (g["y"] < 0) | (g["x"] > width - 1) | (g["y"] > height - 1))
    assert off.sum() >= 20 and (want["val"][off] == KLT_OOB).all()
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    plain, _ = ctx.track(0, 1, fin)
    fallback = live & ~((g["val"] >= 0) & np.isfinite(g["x"]) & np.isfinite(g["y"]))
    assert fallback.sum() >= 20
    assert_records(want[fallback], plain[fallback], c["name"] + ": the composition's fallback is the plain tracker")
    assert_records(run_guess(ctx, fin, g), want, c["name"] + ": mixed list")
    if c["tc"].window_width == 7:
        for i, got in enumerate(run_guess_batch(ctx, fin, g)):
            assert_records(got, want, c["name"] + ": mixed list, batch pair %d" % i)
    again, _ = ctx.track(0, 1, fin)
    assert_records(again, plain, c["name"] + ": the context afterwards")


def test_batch_of_pairs_with_and_without_guesses(ctx):
    """three pairs with different shifts and guesses and one pair without a guess list (entry -1) in one launch = the per-pair calls"""
    tc = shift_case(0)["tc"]
    ctx.configure(tc)
    want, pairs = [], []
    n = 150
    for i, shift in enumerate(((41.3, -27.6), (-35.4, 22.2), (18.7, 44.1), (1.3, -0.8))):
        f0, f1 = large_shift_pair(320, 240, shift, seed=21 + i)
        load_frames(ctx, tc, f0, f1, 10 + 2 * i, 11 + 2 * i)
        fl, _ = ctx.select(10 + 2 * i, n)
        fl["val"][i::19] = -2
        ctx.featbuf_upload(400 + i, fl)
        if i < 3:
            g, _ = noisy_truth(fl, shift, seed=3 + i)
            ctx.featbuf_upload(410 + i, g)
            want.append(ctx.track_guess(10 + 2 * i, 11 + 2 * i, fl, g)[0])
            assert (want[-1]["val"] == KLT_TRACKED).sum() > 30
        else:
            want.append(ctx.track(10 + 2 * i, 11 + 2 * i, fl)[0])
        pairs.append((10 + 2 * i, 11 + 2 * i, 400 + i, 410 + i if i < 3 else -1, 420 + i))
    ctx.track_guess_batch_async(pairs, n)
    ctx.sync()
    for i in range(4):
        assert_records(ctx.featbuf_download(420 + i, n), want[i], "batch pair %d" % i)
    for s in range(10, 18):
        ctx.slot_free(s)


FAR, NEAR = (41.3, -27.6), (12.3, -8.6)


@pytest.mark.parametrize("case_index,max_error,shift", [(0, 0.0, FAR), (0, 1.0, FAR), (0, 1e9, FAR), (1, 1.0, FAR), (2, 1.0, FAR), (0, 1.0, NEAR)],
                         ids=["w7-0", "w7-1", "w7-1e9", "w15-1", "w9-1", "w7-1-near"])
def test_forward_backward_with_guess(ctx, case_index, max_error, shift):
    """an occlusion pair shifted beyond the search range: fwd = G(1, 2, in, guess), back = T(2, 1, fwd), then the rule -- `out` and `back`
    against the oracle composition.  The way back takes no prior, so behind a shift of 41 px it does not come home: with max_error 0 and 1
    the composition rejects every feature the forward run tracked (85 of 85 at window 7), with 1e9 it keeps those the backward run calls
    tracked (54).  With a shift the way back can cover (12.3, -8.6) it keeps 78 of 105, against 70 without the prior."""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, block, n = OCCLUSION_CASES[case_index]
    if case_index == 1:
        width, height, block, n = 320, 240, (70, 170, 100, 220), 150          # (the 15x15 case at the small size)
    f0, f1 = occlusion_pair(width, height, block, shift=shift)
    tc = make_tc(levels=levels, ss=ss, window=window)
    p = params_from_tc(tc)
    fin = ko.select_good_features(p, f0.astype(np.float32), n)
    fin["val"][3::13] = -3
    guess, _ = noisy_truth(fin, shift)
    pyr1, pyr2 = ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))
    want, fwd, wback = fb_guess_compose(ko, p, pyr1, pyr2, fin, guess, max_error)
    tracked = (fin["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
    print("%s, max_error %g: %d tracked forward, %d kept" % (name, max_error, tracked.sum(), (want["val"][tracked] == KLT_TRACKED).sum()))
    assert tracked.sum() > 30
    if max_error == 1e9 or shift == NEAR:
        assert (want["val"][tracked] == KLT_TRACKED).any() and (want["val"][tracked] != KLT_TRACKED).any()
    load_frames(ctx, tc, f0, f1)
    ctx.set_fb_params(max_error=max_error)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, guess)
    ctx.track_fb_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n, FB_BACK)
    ctx.sync()
    assert_records(ctx.featbuf_download(FB_OUT, n), want, name + " out")
    assert_records(ctx.featbuf_download(FB_BACK, n), wback, name + " back")
    ctx.track_fb_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n)                # without the backward records: the same `out`
    ctx.sync()
    assert_records(ctx.featbuf_download(FB_OUT, n), want, name + " out (no back)")
    # the identity guess is klt_track_fb_async
    plain, _, pback = ctx.track_fb(0, 1, fin, want_back=True)
    ctx.track_fb_guess_async(0, 1, FB_IN, FB_IN, FB_OUT, n, FB_BACK)
    ctx.sync()
    assert_records(ctx.featbuf_download(FB_OUT, n), plain, name + " identity out")
    assert_records(ctx.featbuf_download(FB_BACK, n), pback, name + " identity back")


def test_predict_cv(ctx):
    """klt_predict_cv_async = the numpy rule on lists with tracked, lost and freshly replaced slots (1000 records: four workgroups, the last
    one short; the guess buffer is allocated by the call)"""
    rs = np.random.RandomState(7)
    n = 1000
    prev, cur = np.zeros(n, FEAT_DTYPE), np.zeros(n, FEAT_DTYPE)
    for a in (prev, cur):
        a["x"], a["y"] = rs.uniform(0, 2000, n), rs.uniform(0, 1000, n)
    prev["val"][::5] = 1234
    prev["val"][1::7] = -4
    cur["val"][1::7] = 977
    cur["val"][2::9] = -2
    cur["x"][2::9] = cur["y"][2::9] = -1.0
    cur["val"][3::11] = 4321
    prev["aux"], cur["aux"] = 0x21, 0x32
    ctx.featbuf_upload(500, prev)
    ctx.featbuf_upload(501, cur)
    ctx.predict_cv_async(500, 501, 502, n)
    ctx.sync()
    want = predict_cv(prev, cur)
    assert (want["val"] == 0).sum() > 500 and (want["val"] < 0).sum() > 200
    assert_records(ctx.featbuf_download(502, n), want, "predicted")
    assert_records(ctx.featbuf_download(500, n), prev, "prev untouched")
    assert_records(ctx.featbuf_download(501, n), cur, "cur untouched")
    ctx.predict_cv_async(500, 501, 502, 0)                           # nothing to do


def test_error_paths(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError, KltOutOfMemory
    from pyfeaturetrack_amd.backend import Context
    c = shift_case(0)
    fin, guess, n = c["fin"], c["guess"], len(c["fin"])
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, guess)
    ctx.set_fb_params(max_error=1.0)
    with pytest.raises(KltBackendError, match="fb_guess"):                      # the guess list is the output list
        ctx.track_guess_async(0, 1, FB_IN, FB_OUT, FB_OUT, n)
    with pytest.raises(KltBackendError, match="fb_guess"):                      # ... the backward list
        ctx.track_fb_guess_async(0, 1, FB_IN, FB_BACK, FB_OUT, n, FB_BACK)
    with pytest.raises(KltBackendError, match="fb_guess"):                      # ... no feature buffer at all
        ctx.track_guess_async(0, 1, FB_IN, -1, FB_OUT, n)
    ctx.featbuf_alloc(600, 2 * n)
    ctx.featbuf_view(601, 600, 0, n)                                            # two names of the same records
    ctx.featbuf_view(602, 600, 0, n)
    with pytest.raises(KltBackendError, match="fb_guess"):
        ctx.track_guess_async(0, 1, FB_IN, 601, 602, n)
    ctx.featbuf_alloc(610, n - 1)                                               # a guess list one record short, and one never set
    for short in (610, 611):
        with pytest.raises(KltBackendError, match="guess feature buffer"):
            ctx.track_guess_async(0, 1, FB_IN, short, FB_OUT, n)
    with pytest.raises(KltBackendError, match="fb_guess"):                      # a batch: pair 0's guesses are pair 1's output
        ctx.track_guess_batch_async([(0, 1, FB_IN, 620, 621), (0, 1, FB_IN, FB_GUESS, 620)], n)
    for bufs in ((500, 501, 500), (500, 501, 501)):
        with pytest.raises(KltBackendError, match="fb_guess"):
            ctx.predict_cv_async(bufs[0], bufs[1], bufs[2], 10)
    with pytest.raises(KltBackendError, match="not set"):
        ctx.predict_cv_async(630, FB_IN, 631, n)
    ctx.upload(7, c["f0"])                                                      # a frame without pyramids
    with pytest.raises(KltBackendError, match="pyramids"):
        ctx.track_guess_async(0, 7, FB_IN, FB_GUESS, FB_OUT, n)
    with pytest.raises(KltBackendError, match="pyramids"):
        ctx.track_fb_guess_async(0, 7, FB_IN, FB_GUESS, FB_OUT, n, -1)
    ctx.slot_free(7)
    assert_records(run_guess(ctx, fin, guess), c["want"], "the context after the refused calls")
    # every allocation site of one klt_track_guess call refused in turn: KLT_ERR_NOMEM, and the context goes on working.  A fresh context:
    # the call has to allocate its record buffers and the feature order
    fresh = Context(0)
    try:
        load_frames(fresh, c["tc"], c["f0"], c["f1"])
        refused = 0
        for k in range(12):
            fresh.set_option(OPT_FAIL_ALLOC_AFTER, k)
            try:
                out, _ = fresh.track_guess(0, 1, fin, guess)
            except KltOutOfMemory:
                refused += 1
                continue
            finally:
                fresh.set_option(OPT_FAIL_ALLOC_AFTER, -1)
            assert_records(out, c["want"], "after %d refused allocations" % refused)
            break
        else:
            raise AssertionError("the call never got through")
        print("allocations refused in turn: %d" % refused)
        assert refused >= 2
        assert_records(fresh.track_guess(0, 1, fin, guess)[0], c["want"], "context after the walk")
    finally:
        fresh.close()


def test_existing_callers_enqueue_what_they_did(ctx):
    """a klt_track_async run counts one launch of the tracker's timing family and nothing else, with and without guess launches around it;
    a guess launch counts under the same family"""
    c = shift_case(0)
    fin, n = c["fin"], len(c["fin"])
    load_frames(ctx, c["tc"], c["f0"], c["f1"])
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, c["guess"])
    ctx.track_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n)
    ctx.sync()
    try:
        ctx.timing_enable(1)
        ctx.track_async(0, 1, FB_IN, FB_OUT, n)
        ctx.sync()
        assert {k["name"]: k["launches"] for k in ctx.timing_read()} == {"track": 1}
        ctx.timing_enable(1)
        ctx.track_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n)
        ctx.sync()
        assert {k["name"]: k["launches"] for k in ctx.timing_read()} == {"track": 1}
    finally:
        ctx.timing_enable(0)


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


XYV = ("val", "x", "y")


@pytest.mark.parametrize("pillow", [False, True], ids=["numpy", "pillow"])
def test_python_api_pair(pillow):
    """KLTTrackFeatures(..., guess=) on numpy and Pillow frames, with a NaN row, with the forward-backward flag, on foreign feature objects"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        c = shift_case(0)
        f0, f1 = c["f0"], c["f1"]
        if pillow:
            PIL = pytest.importorskip("PIL.Image")
            f0, f1 = PIL.fromarray(f0, "L"), PIL.fromarray(f1, "L")
        tc = make_tc()
        fl = KLTSelectGoodFeatures(tc, f0, 150)
        fin = _records(fl)
        g, _ = noisy_truth(fin, c["shift"])
        positions = np.stack([g["x"], g["y"]], axis=1)
        positions[4::9] = np.nan
        g["val"][4::9] = -1
        want = guess_compose(ko, c["p"], c["pyr1"], c["pyr2"], fin, g)
        KLTTrackFeatures(tc, f0, f1, fl, guess=positions)
        assert_records(_records(fl), want, "KLTTrackFeatures with guess", XYV)
        assert (want["val"] == KLT_TRACKED).sum() > 50

        class Feat:
            pass
        objs = []
        for r in fin:
            o = Feat()
            o.x, o.y, o.val = float(r["x"]), float(r["y"]), int(r["val"])
            o.aff_img = o.aff_img_gradx = o.aff_img_grady = None
            objs.append(o)
        KLTTrackFeatures(tc, f0, f1, objs, guess=positions.tolist())
        assert_records(_records(objs), want, "per-object branch, guess as a list of lists", XYV)
        # with the forward-backward flag
        tcf = make_tc(forwardBackwardCheck=True, fb_max_error=0.75)
        fl = KLTSelectGoodFeatures(tcf, f0, 150)
        wantf, _, wback = fb_guess_compose(ko, c["p"], c["pyr1"], c["pyr2"], fin, g, 0.75)
        KLTTrackFeatures(tcf, f0, f1, fl, guess=positions)
        assert_records(_records(fl), wantf, "with the check", XYV)
        assert_records(np.asarray(tcf.fb_back), wback, "tc.fb_back", XYV)
    finally:
        _restore(old)


def test_python_api_sequential_mode():
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd import synth
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        base = synth.synth_base(320, 240, 21)
        shift = (23.3, -17.6)
        frames = [synth.shift_frame(base, k * shift[0], k * shift[1]) for k in range(3)]
        tc = make_tc(sequentialMode=True)
        p = params_from_tc(tc)
        pyr = [ko.Pyramids(p, f.astype(np.float32)) for f in frames]
        fl = KLTSelectGoodFeatures(tc, frames[0], 150)
        for k in (1, 2):
            fin = _records(fl)
            g, _ = noisy_truth(fin, shift, seed=k)
            want = guess_compose(ko, p, pyr[k - 1], pyr[k], fin, g)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl, guess=np.stack([g["x"], g["y"]], axis=1))
            assert_records(_records(fl), want, "sequential step %d" % k, XYV)
            assert (want["val"] == KLT_TRACKED).sum() > 40
    finally:
        _restore(old)


ACCELERATION = (5.3, 1.7)        # frame k of the clip is the texture moved by k (k + 1) / 2 times this: per-frame shifts of 5.6, 11.1, 16.7, 22.3
                                 # and 27.8 px, the step always inside the search range (15 px), the shift itself outside it from frame 3 on


def accelerating_clip(count=6):
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(320, 240, 21)
    return [synth.shift_frame(base, ACCELERATION[0] * k * (k + 1) / 2, ACCELERATION[1] * k * (k + 1) / 2) for k in range(count)]


def test_sequence_with_prediction_keeps_more_and_equals_the_composition():
    """KLTTrackSequence with tc.motionPrediction on an accelerating pan, without replacement: every row is the CPU composition's (predictor
    rule + oracle steps), and the composition keeps strictly more features than the same loop without the prior"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    old = _quiet()
    try:
        frames = accelerating_clip()
        n = 150
        tc = make_tc(sequentialMode=True)
        p = params_from_tc(tc)
        pyr = [ko.Pyramids(p, f.astype(np.float32)) for f in frames]
        rows = {}
        for mode in (None, "constant_velocity"):
            r = [ko.select_good_features(p, frames[0].astype(np.float32), n)]
            for k in range(1, len(frames)):
                g = predict_cv(r[-2], r[-1]) if mode and k >= 2 else None
                r.append(guess_compose(ko, p, pyr[k - 1], pyr[k], r[-1], g))
            rows[mode] = r
        kept = {mode: int((r[-1]["val"] >= 0).sum()) for mode, r in rows.items()}
        print("features left after %d frames: %d without the prior, %d with it" % (len(frames), kept[None], kept["constant_velocity"]))
        assert kept["constant_velocity"] > kept[None]
        for mode in (None, "constant_velocity"):
            got = KLTTrackSequence(make_tc(sequentialMode=True, motionPrediction=mode), iter(frames), n, replace_lost=False)
            for k, want in enumerate(rows[mode]):
                for name, col in (("val", got.val), ("x", got.x), ("y", got.y)):
                    assert np.array_equal(col[k], want[name]), (mode, k, name)
    finally:
        _restore(old)


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "in-order"])
@pytest.mark.parametrize("fb", [False, True], ids=["plain", "fb"])
def test_sequence_equals_the_host_loop(prefetch, fb):
    """... and with replacement (and the forward-backward check): the table equals the per-frame host loop built from the same pieces --
    KLTPredictConstantVelocity, KLTTrackFeatures(guess=), KLTReplaceLostFeatures -- bit for bit"""
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, storeFeatures as sf, trackFeatures as tf
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    old = _quiet()
    try:
        frames = accelerating_clip()
        n = 150

        def make(mode="constant_velocity"):
            return make_tc(sequentialMode=True, forwardBackwardCheck=fb, motionPrediction=mode)
        tc = make()
        want = sf.KLTCreateFeatureTable(len(frames), n)
        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
        sf.KLTStoreFeatureList(fl, want, 0)
        before = None
        for k in range(1, len(frames)):
            guess = tf.KLTPredictConstantVelocity(before, fl) if k >= 2 else None
            before = _records(fl)
            tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl, guess=guess)
            sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
            sf.KLTStoreFeatureList(fl, want, k)
        got = KLTTrackSequence(make(), iter(frames), n, prefetch=prefetch)
        assert np.array_equal(got.val, want.val) and np.array_equal(got.x, want.x) and np.array_equal(got.y, want.y)
        plain = KLTTrackSequence(make(None), iter(frames), n, prefetch=prefetch)
        assert not (np.array_equal(plain.val, want.val) and np.array_equal(plain.x, want.x))
    finally:
        _restore(old)


def test_affine_check_takes_no_guess():
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    old = _quiet()
    try:
        c = shift_case(0)
        tc = make_tc(affineConsistencyCheck=2)
        fl = KLTSelectGoodFeatures(tc, c["f0"], 40)
        with pytest.raises(ValueError, match="guess"):
            KLTTrackFeatures(tc, c["f0"], c["f1"], fl, guess=np.zeros((40, 2), np.float32))
        KLTTrackFeatures(tc, c["f0"], c["f0"], fl)                   # the context works on
    finally:
        _restore(old)
