"""Track identities through the Python API: KLTTrackSequence under tc.reacquireLost in its four arrangements
(prefetch x replace_lost), KLTUpdateIdentities in the reference's per-frame loop and adopted frames behind the CLAHE stage, each against
the rule in numpy (tests/reacquire_expected.py) applied to the lists the device produced; the known answer of the clip, computed on the
CPU from the oracle's lists; the switch off; the refusals of the Python layer; examples/reacquire_sequence.py.

The clip is the drifting scene of examples/reacquire.py (drift (1.0, 0.5) px per frame), 160 x 120, 12 frames, 120 features asked for,
a flat block over its middle in frames 3 .. 7."""
import os
import sys
import threading

import numpy as np
import pytest

import reacquire_expected as R
from conftest import REPO

pytestmark = pytest.mark.gpu
N = 120
# The known answer, from the CPU alone: the restatement on the lists of oracle/klt_oracle.py (select, track, replace) for this clip --
# (identities of frame 0 alive in the last frame, re-acquired ones among them, of those more than 2 px from their own corner, the
# largest gap of any re-acquisition) -- with replacement and without.  The two conditions the issue sets hold for them: a re-acquisition
# with gap >= 3 (the largest is 5: under the block from frame 3 to 7), at most a tenth of the re-acquired on a wrong corner (1 of 10).
KNOWN = {True: (19, 10, 1, 5), False: (9, 0, 0, -1)}
ALIVE_WITHOUT = 9                                            # slots tracked without a break from frame 0 to frame 11


@pytest.fixture(scope="module")
def clip():
    return R.occluded_clip()


@pytest.fixture()
def quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf
    from pyfeaturetrack_amd import trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    yield
    sgf.KLT_verbose, tf.KLT_verbose = old


def _tc(**attrs):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    tc = KLT_TrackingContext()
    tc.mindist, tc.max_residue = 12, 10.0
    for k, v in attrs.items():
        setattr(tc, k, v)
    return tc


def _rule(frames, lists, tc):
    from pyfeaturetrack_amd.params import reacquire_params_from_tc
    tc.reacquireLost, was = True, tc.reacquireLost
    params = reacquire_params_from_tc(tc)
    tc.reacquireLost = was
    rows, _ = R.run_sequence(frames, [np.ascontiguousarray(row).view(R.FEAT_DTYPE) for row in lists],
                             mode=R.UPRIGHT + bool(tc.descriptorOrientation), **params)
    return rows


def test_the_known_answer_meets_the_conditions_on_the_cpu(clip):
    """the constants above, recomputed from the oracle's lists; and the two conditions the clip must meet"""
    from pyfeaturetrack_amd.params import params_from_tc
    tc = _tc(reacquireLost=True)
    for replace in (True, False):
        lists = R.oracle_lists(params_from_tc(tc), clip, N, replace)
        ident = _rule(clip, lists, tc)
        assert R.clip_counts(lists, ident, N) == KNOWN[replace]
    alive, regained, wrong, gap = KNOWN[True]
    assert gap >= 3 and 10 * wrong <= regained and alive > ALIVE_WITHOUT


@pytest.mark.parametrize("replace", [True, False], ids=["replace", "keep"])
@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "plain"])
def test_track_sequence_equals_the_rule_and_the_known_answer(clip, quiet, prefetch, replace):
    import pyfeaturetrack_amd as klt
    from pyfeaturetrack_amd.backend import IDENT_DTYPE
    tc = _tc(reacquireLost=True)
    ft = klt.KLTTrackSequence(tc, clip, N, replace_lost=replace, prefetch=prefetch)
    assert ft.ident.dtype == IDENT_DTYPE and ft.ident.shape == (len(clip), N)
    want = _rule(clip, ft.rec, tc)
    assert ft.ident.view(R.IDENT_DTYPE).tobytes() == want.tobytes(), np.argwhere(ft.ident.view(R.IDENT_DTYPE) != want)[:5]
    assert R.clip_counts(ft.rec, ft.ident, N) == KNOWN[replace]


def test_other_switches_and_parameters(clip, quiet):
    """steered descriptors, a small bank, no gate, no ratio test, a short memory; beside the forward-backward check and the crowding check"""
    import pyfeaturetrack_amd as klt
    tc = _tc(reacquireLost=True, descriptorOrientation=True, reacquire_capacity=8, reacquire_radius=None, reacquire_ratio=None,
             reacquire_max_gap=2, reacquire_max_distance=40, forwardBackwardCheck=True, crowdingCheck=True)
    ft = klt.KLTTrackSequence(tc, clip, N)
    assert ft.ident.view(R.IDENT_DTYPE).tobytes() == _rule(clip, ft.rec, tc).tobytes()
    assert ft.ident["gap"].max() <= 2 and ft.crowd.shape == ft.ident.shape


def test_switch_off_leaves_no_trace(clip, quiet):
    """on a thread of its own -- a context nobody has used: no `ident`, and the path diagnostic stays 0"""
    import pyfeaturetrack_amd as klt
    from pyfeaturetrack_amd.backend import context_of
    seen = {}

    def run():
        tc = _tc()
        ft = klt.KLTTrackSequence(tc, clip[:4], N)
        ctx = context_of(tc)
        seen["ident"], seen["path"] = hasattr(ft, "ident"), ctx.reacquire_path()
    t = threading.Thread(target=run)
    t.start()
    t.join()
    assert seen == {"ident": False, "path": 0}


def test_update_identities_in_the_per_frame_loop(clip, quiet):
    import pyfeaturetrack_amd as klt
    from pyfeaturetrack_amd.selectGoodFeatures import features_to_array
    tc = _tc()                                               # (tc.reacquireLost is KLTTrackSequence's switch: not asked here)
    for again in range(2):                                   # the second pass begins anew after KLTResetIdentities
        fl = klt.KLTSelectGoodFeatures(tc, clip[0], N)
        lists, got = [features_to_array(fl).copy()], [klt.KLTUpdateIdentities(tc, clip[0], fl)]
        for k in range(1, len(clip)):
            klt.KLTTrackFeatures(tc, clip[k - 1], clip[k], fl)
            klt.KLTReplaceLostFeatures(tc, clip[k], fl)
            lists.append(features_to_array(fl).copy())
            got.append(klt.KLTUpdateIdentities(tc, clip[k], fl if k % 2 else lists[-1]))       # a feature list or its records
        got = np.stack(got)
        assert got.view(R.IDENT_DTYPE).tobytes() == _rule(clip, lists, tc).tobytes()
        assert R.clip_counts(np.stack(lists), got, N) == KNOWN[True]
        with pytest.raises(ValueError, match="the sequence began with"):
            klt.KLTUpdateIdentities(tc, clip[-1], lists[-1][:5])
        klt.KLTResetIdentities(tc)


def test_python_refusals_come_before_any_device_work(clip, quiet):
    import pyfeaturetrack_amd as klt
    text = "descriptors take single-channel 8-bit frames"
    with pytest.raises(ValueError, match=text):
        klt.KLTTrackSequence(_tc(reacquireLost=True), [f.astype(np.float32) for f in clip[:3]], N)
    from PIL import Image
    with pytest.raises(ValueError, match=text):
        klt.KLTTrackSequence(_tc(reacquireLost=True), [Image.fromarray(np.dstack([f] * 3)) for f in clip[:3]], N)      # a colour clip
    with pytest.raises(ValueError, match=text):
        klt.KLTTrackSequence(_tc(reacquireLost=True), [clip[0], clip[1], clip[2].astype(np.float32)], N)      # a later frame
    with pytest.raises(ValueError, match="reacquire_capacity"):
        klt.KLTTrackSequence(_tc(reacquireLost=True, reacquire_capacity=100), iter(()), N)     # (the frames are never asked for)
    with pytest.raises(TypeError, match="reacquire_max_gap"):
        klt.KLTTrackSequence(_tc(reacquireLost=True, reacquire_max_gap=1.5), iter(()), N)
    with pytest.raises(ValueError, match="reacquireLost"):
        klt.KLTTrackSequence(_tc(reacquireLost="on"), iter(()), N)
    with pytest.raises(ValueError, match=text):
        klt.KLTUpdateIdentities(_tc(), clip[0].astype(np.float32), np.zeros(3, R.FEAT_DTYPE))
    with pytest.raises(ValueError, match="at least one feature"):
        klt.KLTUpdateIdentities(_tc(), clip[0], np.zeros(0, klt.trackIdentities.FEAT_DTYPE))


def test_adopted_frames_behind_the_clahe_stage(clip):
    """frames that live in device memory (klt_slot_adopt_u8) with tc.equalization on: the identities describe the equalised frame"""
    from pyfeaturetrack_amd.backend import Context, FEAT_DTYPE
    from pyfeaturetrack_amd.params import equalize_params_from_tc, params_from_tc
    import equalize_expected as ee
    tc = _tc(equalization="clahe")
    lists = R.oracle_lists(params_from_tc(_tc()), clip[:6], N)       # any lists do: the oracle's of the plain clip
    eq = equalize_params_from_tc(tc)
    frames = [ee.clahe(f, eq.tiles_x, eq.tiles_y, eq.clip_q8) for f in clip[:6]]
    want, _ = R.run_sequence(frames, list(lists), capacity=64, max_gap=30, radius=24)
    ctx = Context(0)
    dev = []
    try:
        ctx.set_params(params_from_tc(tc))
        ctx.set_equalize_params(eq)
        ctx.set_reacquire_params(capacity=64)
        h, w = clip[0].shape
        for k in range(6):
            dev.append(ctx.device_alloc(w * h))
            ctx.device_write(dev[-1], clip[k])
            ctx.adopt_u8(k % 2, dev[-1], w, h)
            ctx.featbuf_upload(10, lists[k].astype(FEAT_DTYPE))
            if k == 0:
                ctx.reacquire_begin_async(0, 10, 11, N)
            else:
                ctx.reacquire_step_async(k % 2, 10, 11 + (k - 1) % 2, 11 + k % 2, N)
            got = ctx.ident_download(11 + k % 2, N).view(R.IDENT_DTYPE)
            assert got.tobytes() == want[k].tobytes(), k
    finally:
        for k in range(2):
            ctx.slot_free(k)
        for d in dev:
            ctx.device_free(d)
        ctx.close()


def test_example_reacquire_sequence(quiet):
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import reacquire_sequence
    finally:
        sys.path.pop(0)
    res = reacquire_sequence.main(["--size", "160x120", "--features", "120", "--frames", "12", "--cover", "3:8"])
    assert res[True][0] > res[False][0] and res[True][:3] == KNOWN[True][:3] and res[False][0] == ALIVE_WITHOUT
