"""Per-feature track quality (klt_track_quality*) on the device against the numpy restatement of the rule
(tests/quality_expected.py).  Every comparison is exact on all four fields -- residue, ncc, min_eig and val; a difference is a bug in the
kernel or in the restatement's transcription of the rule, not a tolerance."""
import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from light_expected import edge_features, lit_pair
from quality_expected import (FEAT_DTYPE, KLT_LARGE_RESIDUE, KLT_TRACKED, QUALITY_DTYPE, quality_expected, shifted_case, unmeasured_kinds)

pytestmark = pytest.mark.gpu

FB_IN, FB_OUT, FB_Q = 100, 101, 102
FIELDS = ("val", "residue", "ncc", "min_eig")


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def assert_quality(got, want, what):
    assert got.dtype == QUALITY_DTYPE and len(got) == len(want), what
    for name in FIELDS:
        # bit patterns: NaN would equal NaN, -0 would differ from +0
        g, w = got[name].view(np.uint32 if name != "val" else np.int32), want[name].view(np.uint32 if name != "val" else np.int32)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s.%s: %d of %d differ, first at %d: got %r, want %r (records %r / %r)" % (
            what, name, bad.size, len(got), bad[0], got[name][bad[0]], want[name][bad[0]], got[bad[0]], want[bad[0]])


def same_bytes(a, b):
    """record arrays compared as bytes: the lists hold NaN coordinates"""
    return a.tobytes() == b.tobytes()


_PAIRS = {}


def pair_case(width, height, window, seed=5):
    """(tc, params, frames, oracle pyramids, list) of the shifted pair at one size and window: subsampling 2, 2 levels up to 9x9 and 1
    above (the quality launch reads level 0 alone; under two levels a 31x31 tracker keeps none of the list at 160x120), 300 records on a
    jittered grid that reaches every edge, a few of them at integer coordinates.  Computed once, read-only."""
    key = (width, height, window, seed)
    if key not in _PAIRS:
        from oracle import klt_oracle as ko
        tc = make_tc(levels=2 if window <= 9 else 1, ss=2, window=window)
        p = params_from_tc(tc)
        f1, f2 = lit_pair(width, height, gain=1.0, offset=0.0)
        fin = edge_features(width, height, 300, seed)
        fin["x"][3::17] = np.floor(fin["x"][3::17])              # positions with integer coordinates
        fin["y"][3::17] = np.floor(fin["y"][3::17])
        fin["x"][5::29] = np.floor(fin["x"][5::29])              # ... and with one of them
        pyr1, pyr2 = ko.Pyramids(p, f1.astype(np.float32)), ko.Pyramids(p, f2.astype(np.float32))
        for a in (f1, f2, fin):
            a.setflags(write=False)
        _PAIRS[key] = dict(tc=tc, p=p, f1=f1, f2=f2, fin=fin, pyr1=pyr1, pyr2=pyr2, w=window, size=(width, height))
    return _PAIRS[key]


def load(ctx, c, s0=0, s1=1):
    ctx.configure(c["tc"])
    ctx.set_light_params(mode=0)
    ctx.upload(s0, c["f1"])
    ctx.upload(s1, c["f2"])
    ctx.build_pyramids(s0)
    ctx.build_pyramids(s1)


def lists_of(ctx, c, s0=0, s1=1, start=120):
    """`in` = the case's list, `out` = what the device tracker makes of it, with 82 records from `start` on overwritten by the kinds the
    rule does not measure (and the last window positions it does)"""
    out, _ = ctx.track(s0, s1, c["fin"])
    width, height = c["size"]
    return unmeasured_kinds(c["fin"], out, c["w"], width, height, start=start)


WINDOW_CASES = [(7, 160, 120), (15, 160, 120), (5, 160, 120), (9, 160, 120), (17, 160, 120), (31, 160, 120), (7, 251, 187)]


@pytest.mark.parametrize("window,width,height", WINDOW_CASES, ids=["w%d_%dx%d" % c for c in WINDOW_CASES])
def test_kernel_equals_the_rule(ctx, window, width, height):
    """compile-time windows 7 and 15, run-time windows 5, 9, 17 and 31 (one per samples-per-lane class), a frame of odd size: 300 records,
    `out` from a device tracker launch, every unmeasured kind among them; then n = 1"""
    from oracle import klt_oracle as ko
    c = pair_case(width, height, window)
    load(ctx, c)
    fin, fout, kinds = lists_of(ctx, c)
    want = quality_expected(ko, c["pyr1"], c["pyr2"], fin, fout, window)
    for i, is_measured in kinds.items():
        assert want["val"][i] == int(is_measured), (i, fin[i], fout[i])
    rest = np.ones(len(fin), bool)
    rest[list(kinds)] = False
    print("window %d: %d measured, %d of them tracker outputs" % (window, (want["val"] == 1).sum(), (want["val"][rest] == 1).sum()))
    assert (want["val"][rest] == 1).sum() >= 40                                # records the tracker itself produced
    assert (want["val"][rest] == 0).sum() >= 20                                  # ... and lost
    got = ctx.track_quality(0, 1, fin, fout)
    assert_quality(got, want, "window %d" % window)
    one = int(np.flatnonzero(rest & (want["val"] == 1))[0])
    got = ctx.track_quality(0, 1, fin[one:one + 1], fout[one:one + 1])
    assert_quality(got, want[one:one + 1], "n = 1")
    empty = ctx.track_quality(0, 1, fin[:0], fout[:0])                          # n = 0: KLT_OK, nothing enqueued
    assert len(empty) == 0


def test_residue_is_the_number_max_residue_tests_on_the_device(ctx):
    """ctx.track without max_residue, then with max_residue = the median measured residue of the tracked features: a feature tracked in
    the first run is KLT_LARGE_RESIDUE in the second iff its residue > float32(r), else KLT_TRACKED"""
    from oracle import klt_oracle as ko
    c = shifted_case()
    fin = c["fin"]
    load(ctx, c)
    first, _ = ctx.track(0, 1, fin)
    q = ctx.track_quality(0, 1, fin, first)
    assert_quality(q, quality_expected(ko, c["pyr1"], c["pyr2"], fin, first, 7), "the shifted pair")
    tracked = first["val"] == KLT_TRACKED
    assert tracked.sum() >= 200 and np.array_equal(q["val"] == 1, tracked)
    r = np.float32(np.median(q["residue"][tracked]))
    ctx.configure(make_tc(levels=2, ss=4, window=7, max_residue=float(r)))
    assert ctx.pyramids_valid(0) and ctx.pyramids_valid(1)
    second, _ = ctx.track(0, 1, fin)
    large = q["residue"] > r
    assert (large & tracked).sum() >= 50 and (~large & tracked).sum() >= 50
    assert (second["val"][tracked & large] == KLT_LARGE_RESIDUE).all()
    assert (second["val"][tracked & ~large] == KLT_TRACKED).all()
    assert np.array_equal(second["x"][tracked & ~large], first["x"][tracked & ~large])


@pytest.mark.parametrize("window", [7, 9])
def test_batched_pairs_equal_their_single_calls(ctx, window):
    """two pairs in one launch, the second with the frames the other way round and another list: each pair's records are its single
    call's and the rule's"""
    from oracle import klt_oracle as ko
    a = pair_case(160, 120, window)
    b = pair_case(160, 120, window, seed=9)
    n = len(a["fin"])
    load(ctx, a, 0, 1)
    ctx.upload(2, a["f2"])
    ctx.upload(3, a["f1"])
    ctx.build_pyramids(2)
    ctx.build_pyramids(3)
    try:
        in_a, out_a, _ = lists_of(ctx, a, 0, 1)
        in_b, out_b, _ = lists_of(ctx, b, 2, 3, start=40)
        want_a = quality_expected(ko, a["pyr1"], a["pyr2"], in_a, out_a, window)
        want_b = quality_expected(ko, a["pyr2"], a["pyr1"], in_b, out_b, window)
        assert (want_b["val"] == 1).sum() >= 40 and not np.array_equal(want_a, want_b)
        single_a, single_b = ctx.track_quality(0, 1, in_a, out_a), ctx.track_quality(2, 3, in_b, out_b)
        for fb, fl in ((300, in_a), (301, out_a), (310, in_b), (311, out_b)):
            ctx.featbuf_upload(fb, fl)
        for rep in range(2):                    # the second launch finds its descriptor table on the device
            ctx.track_quality_batch_async([(0, 1, 300, 301, 302), (2, 3, 310, 311, 312)], n)
            got_a, got_b = ctx.quality_download(302, n), ctx.quality_download(312, n)
            assert_quality(got_a, single_a, "pair 0 against its single call")
            assert_quality(got_b, single_b, "pair 1 against its single call")
            assert_quality(got_a, want_a, "pair 0 against the rule")
            assert_quality(got_b, want_b, "pair 1 against the rule")
        ctx.track_quality_batch_async([(2, 3, 310, 311, 302), (0, 1, 300, 301, 312)], n)      # another table: the pairs swapped
        assert_quality(ctx.quality_download(302, n), want_b, "pair 1 first")
        assert_quality(ctx.quality_download(312, n), want_a, "pair 0 second")
    finally:
        ctx.slot_free(2)
        ctx.slot_free(3)


def test_light_mode_changes_nothing(ctx):
    """with klt_set_light_params mode 1 the quality records are those of mode 0"""
    from oracle import klt_oracle as ko
    c = pair_case(160, 120, 7)
    load(ctx, c)
    fin, fout, _ = lists_of(ctx, c)
    want = quality_expected(ko, c["pyr1"], c["pyr2"], fin, fout, 7)
    plain = ctx.track_quality(0, 1, fin, fout)
    try:
        ctx.set_light_params(mode=1)
        lit = ctx.track_quality(0, 1, fin, fout)
        ctx.featbuf_upload(FB_IN, fin)
        ctx.featbuf_upload(FB_OUT, fout)
        ctx.track_quality_batch_async([(0, 1, FB_IN, FB_OUT, FB_Q)], len(fin))
        batched = ctx.quality_download(FB_Q, len(fin))
    finally:
        ctx.set_light_params(mode=0)
    assert_quality(plain, want, "mode 0")
    assert_quality(lit, want, "mode 1")
    assert_quality(batched, want, "mode 1, batched")


def test_refused_arguments_enqueue_nothing(ctx):
    """fb_quality that is fb_in or fb_out -- by index, or by address through a view --, a slot without pyramids, a slot that was never
    filled: each returns its error, no buffer changes, and the context measures correctly afterwards"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd._abi import KltBackendError
    c = pair_case(160, 120, 7)
    load(ctx, c)
    fin, fout, _ = lists_of(ctx, c)
    n = len(fin)
    want = quality_expected(ko, c["pyr1"], c["pyr2"], fin, fout, 7)
    sentinel = np.zeros(n, FEAT_DTYPE)
    sentinel["x"], sentinel["val"], sentinel["aux"] = 12345.0, 77, -9
    VIEW_IN, VIEW_OUT, RAW = 110, 111, 5
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_OUT, fout)
    ctx.featbuf_upload(FB_Q, sentinel)
    ctx.featbuf_view(VIEW_IN, FB_IN, 0, n)                   # second names of the two lists
    ctx.featbuf_view(VIEW_OUT, FB_OUT, 0, n)
    ctx.upload(RAW, c["f2"])                                 # a frame without pyramids
    assert not ctx.pyramids_valid(RAW)
    refused = [
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, FB_IN, n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, FB_OUT, n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, VIEW_IN, n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, VIEW_OUT, n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, -1, n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_batch_async([(0, 1, FB_IN, FB_OUT, FB_Q), (0, 1, FB_IN, FB_Q, 120)], n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_batch_async([(0, 1, FB_IN, FB_OUT, FB_Q), (0, 1, FB_IN, FB_OUT, FB_Q)], n)),
        (r"error -1: .*fb_quality", lambda: ctx.track_quality_batch_async([(0, 1, FB_IN, FB_OUT, FB_Q), (0, 1, FB_IN, FB_OUT, VIEW_IN)], n)),
        (r"error -3: .*pyramids", lambda: ctx.track_quality_async(0, RAW, FB_IN, FB_OUT, FB_Q, n)),
        (r"error -3: .*pyramids", lambda: ctx.track_quality_async(RAW, 1, FB_IN, FB_OUT, FB_Q, n)),
        (r"error -3: .*pyramids", lambda: ctx.track_quality_batch_async([(0, 1, FB_IN, FB_OUT, FB_Q), (0, RAW, FB_IN, FB_OUT, 120)], n)),
        (r"error -3: .*pyramids", lambda: ctx.track_quality(0, RAW, fin, fout)),
        (r"error -", lambda: ctx.track_quality_async(0, 9, FB_IN, FB_OUT, FB_Q, n)),                  # a slot that was never filled
        (r"error -3: .*feature buffer", lambda: ctx.track_quality_async(0, 1, 130, FB_OUT, FB_Q, n)),  # a list that does not exist
        (r"error -1: ", lambda: ctx.track_quality_async(0, 1, FB_IN, FB_OUT, FB_Q, -1)),
    ]
    try:
        for pattern, call in refused:
            with pytest.raises(KltBackendError, match=pattern):
                call()
            ctx.sync()
            assert same_bytes(ctx.featbuf_download(FB_Q, n), sentinel), pattern              # nothing was written
            assert same_bytes(ctx.featbuf_download(FB_IN, n), fin) and same_bytes(ctx.featbuf_download(FB_OUT, n), fout), pattern
        ctx.track_quality_async(0, 1, FB_IN, FB_OUT, FB_Q, 0)                               # n == 0: KLT_OK, nothing enqueued
        ctx.sync()
        assert same_bytes(ctx.featbuf_download(FB_Q, n), sentinel)
        ctx.track_quality_async(0, 1, VIEW_IN, VIEW_OUT, FB_Q, n)                           # views as lists are fine
        assert_quality(ctx.quality_download(FB_Q, n), want, "the context after the refused calls")
        assert_quality(ctx.track_quality(0, 1, fin, fout), want, "klt_track_quality after the refused calls")
    finally:
        ctx.slot_free(RAW)


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


_CLIP = {}


def clip_case():
    """6 frames of 160x120 moving by (1.3, -0.8) a frame, their oracle pyramids (7x7, 2 levels, subsampling 2)"""
    if not _CLIP:
        from oracle import klt_oracle as ko
        from pyfeaturetrack_amd import synth
        base = synth.synth_base(160, 120, 11)
        frames = [synth.synth_frame(160, 120, 11, k, shift=(1.3, -0.8), base=base) for k in range(6)]
        p = params_from_tc(make_tc(levels=2, ss=2, window=7))
        _CLIP.update(frames=frames, p=p, pyr=[ko.Pyramids(p, f.astype(np.float32)) for f in frames])
    return _CLIP


def _load_clip(ctx, tc, frames):
    ctx.configure(tc)
    ctx.set_light_params(mode=0)
    for k, f in enumerate(frames):
        ctx.upload(10 + k, f)
        ctx.build_pyramids(10 + k)


def _free_clip(ctx, frames):
    for k in range(len(frames)):
        ctx.slot_free(10 + k)


@pytest.mark.parametrize("check", [None, "forwardBackwardCheck"])
def test_track_features_leaves_quality_last(ctx, check):
    """KLTTrackFeatures with tc.trackQuality over 6 frames in sequential mode, lost features replaced after every step: tc.quality_last is
    Context.track_quality on the records before and after the call, and the rule; without the switch nothing is left"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    c = clip_case()
    frames, n = c["frames"], 120
    old = _quiet()
    try:
        tc = make_tc(levels=2, ss=2, window=7, sequentialMode=True)
        if check:
            setattr(tc, check, True)
        off = make_tc(levels=2, ss=2, window=7)
        fl = KLTSelectGoodFeatures(off, frames[0], n)
        KLTTrackFeatures(off, frames[0], frames[1], fl)
        assert not hasattr(off, "quality_last")                # off by default: nothing new
        fl = KLTSelectGoodFeatures(tc, frames[0], n)
        tc.trackQuality = True
        _load_clip(ctx, make_tc(levels=2, ss=2, window=7), frames)
        measured = lost = refilled = 0
        for k in range(1, len(frames)):
            before = _records(fl)
            KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            after = _records(fl)
            q = tc.quality_last
            assert q.dtype == QUALITY_DTYPE and len(q) == n
            assert_quality(q, ctx.track_quality(10 + k - 1, 10 + k, before, after), "step %d against Context.track_quality" % k)
            assert_quality(q, quality_expected(ko, c["pyr"][k - 1], c["pyr"][k], before, after, 7), "step %d against the rule" % k)
            assert np.array_equal(q["val"] == 1, (before["val"] >= 0) & (after["val"] == KLT_TRACKED))
            measured += int((q["val"] == 1).sum())
            lost += int(((before["val"] >= 0) & (after["val"] < 0)).sum())
            refilled += int((before["val"] > 0).sum()) if k >= 2 else 0
            KLTReplaceLostFeatures(tc, frames[k], fl)
        # (the oracle on this clip: 78 of the 120 slots can be filled at this size, 71 are tracked and about 7 lost and refilled per step)
        assert measured >= 250 and lost >= 20 and refilled >= 15, (measured, lost, refilled)
    finally:
        _restore(old)
        _free_clip(ctx, frames)


@pytest.mark.parametrize("prefetch", [True, False])
def test_track_sequence_carries_the_quality_table(ctx, prefetch):
    """KLTTrackSequence with tc.trackQuality, 6 frames, lost features replaced: row k of ft.quality is Context.track_quality on rows k - 1
    and k of the table, and the rule (a slot the replacement refilled is not measured: it was lost when the launch ran); row 0 is all
    zero; the feature records are those of a call without the switch"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    c = clip_case()
    frames, n = c["frames"], 120
    old = _quiet()
    try:
        tc = make_tc(levels=2, ss=2, window=7)
        plain = KLTTrackSequence(tc, frames, n, prefetch=prefetch)
        assert plain.quality is None
        tc.trackQuality = True
        ft = KLTTrackSequence(tc, frames, n, prefetch=prefetch)
        assert np.array_equal(ft.rec, plain.rec)
        q = ft.quality
        assert q.shape == (len(frames), n) and q.dtype == QUALITY_DTYPE
        assert not q[0].view(np.uint32).any()
        _load_clip(ctx, make_tc(levels=2, ss=2, window=7), frames)
        refilled = 0
        for k in range(1, len(frames)):
            before, after = np.ascontiguousarray(ft.rec[k - 1]), np.ascontiguousarray(ft.rec[k])
            assert_quality(np.ascontiguousarray(q[k]), ctx.track_quality(10 + k - 1, 10 + k, before, after), "row %d against Context.track_quality" % k)
            assert_quality(np.ascontiguousarray(q[k]), quality_expected(ko, c["pyr"][k - 1], c["pyr"][k], before, after, 7), "row %d against the rule" % k)
            refilled += int((after["val"] > 0).sum())
            assert (q[k]["val"][after["val"] > 0] == 0).all()
            assert (q[k]["val"] == 1).sum() >= n // 2
        assert refilled >= 15
    finally:
        _restore(old)
        _free_clip(ctx, frames)
