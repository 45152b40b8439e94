"""tc.equalization = "clahe" through the Python API: every call equals the same call with the switch off on frames
equalised on the host by the rule (tests/equalize_expected.py) -- KLTSelectGoodFeatures, KLTTrackFeatures in both modes and with the other
switches, KLTReplaceLostFeatures, KLTTrackSequence; toggling the switch and the tile grid between calls on the same frame objects; the
frames the switch takes; KLTEqualizeImage.  Comparisons are on bytes."""
import os

import numpy as np
import pytest

import equalize_expected as ee
from conftest import GOLDEN, read_pgm
from helpers import make_tc

pytestmark = pytest.mark.gpu
NFEAT = 150
_FRAMES = {}


def pair():
    """the 320 x 240 golden pair with its left half darkened"""
    if "pair" not in _FRAMES:
        _FRAMES["pair"] = [ee.darken_left_half(read_pgm(os.path.join(GOLDEN, name))) for name in ("img0.pgm", "img1.pgm")]
        for f in _FRAMES["pair"]:
            f.setflags(write=False)
    return _FRAMES["pair"]


def clip():
    """six frames of a shifting texture, left half darkened"""
    if "clip" not in _FRAMES:
        from pyfeaturetrack_amd import synth
        base = synth.synth_base(320, 240, 7)
        _FRAMES["clip"] = [ee.darken_left_half(synth.shift_frame(base, 1.3 * k, -0.8 * k)) for k in range(6)]
    return _FRAMES["clip"]


def equalised(frames, tiles=(8, 8), clip_limit=3.0):
    key = ("eq", id(frames), tiles, clip_limit)
    if key not in _FRAMES:
        _FRAMES[key] = [ee.clahe(f, tiles[0], tiles[1], ee.clip_q8_of(clip_limit)) for f in frames]
    return _FRAMES[key]


@pytest.fixture(autouse=True)
def quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    yield
    sgf.KLT_verbose, tf.KLT_verbose = old


def _tc(**attrs):
    return make_tc(**attrs)


def _records(fl):
    return np.array([(f.x, f.y, f.val) for f in fl], np.float64)


def _same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), "%s: %d of %d records differ" % (
        what, int((got != want).any(axis=1).sum()) if got.shape == want.shape else -1, len(want))


def _steps(tc, frames, sequential):
    """select on frame 0, track 0 -> 1, replace on frame 1, track 1 -> 0 (ping-pong) or 1 -> 1 shifted back (sequential: frame 0 again):
    the records after every call, and what the switches of the call left on the tracking context"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    out = []
    fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
    out.append(("selected", _records(fl)))
    KLTTrackFeatures(tc, frames[0], frames[1], fl)
    out.append(("tracked", _records(fl)))
    for name in ("quality_last", "fb_back"):
        if getattr(tc, name, None) is not None and (name != "fb_back" or getattr(tc, "forwardBackwardCheck", False)):
            out.append((name, np.frombuffer(np.asarray(getattr(tc, name)).tobytes(), np.uint8)[:, None]))
    KLTReplaceLostFeatures(tc, frames[1], fl)
    out.append(("replaced", _records(fl)))
    KLTTrackFeatures(tc, frames[1], frames[0], fl)
    out.append(("tracked back", _records(fl)))
    return out


@pytest.mark.parametrize("extra", [{}, {"lightingCompensation": "gain_bias"}, {"forwardBackwardCheck": True}, {"smoothBeforeSelecting": False}],
                         ids=["plain", "gain_bias", "forward_backward", "raw_selection"])
@pytest.mark.parametrize("sequential", [False, True], ids=["pingpong", "sequential"])
def test_calls_equal_their_host_equalised_twins(sequential, extra):
    frames = pair()
    on = _steps(_tc(sequentialMode=sequential, trackQuality=True, equalization="clahe", **extra), frames, sequential)
    twin = _steps(_tc(sequentialMode=sequential, trackQuality=True, **extra), equalised(frames), sequential)
    assert [n for n, _ in on] == [n for n, _ in twin]
    for (name, got), (_, want) in zip(on, twin):
        _same(got, want, name)
    selected = on[0][1]
    assert (selected[:, 2] >= 0).sum() == NFEAT
    # ... and it is not the call without the switch
    off = _steps(_tc(sequentialMode=sequential, trackQuality=True, **extra), frames, sequential)
    assert off[0][1].tobytes() != selected.tobytes()


@pytest.mark.parametrize("prefetch", [True, False], ids=["prefetch", "plain"])
def test_sequence_equals_its_host_equalised_twin(prefetch):
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = clip()
    on = KLTTrackSequence(_tc(equalization="clahe", clahe_tiles=(6, 4), clahe_clip_limit=2.0), frames, NFEAT, replace_lost=True, prefetch=prefetch)
    twin = KLTTrackSequence(_tc(), equalised(frames, (6, 4), 2.0), NFEAT, replace_lost=True, prefetch=prefetch)
    assert on.rec.shape == (6, NFEAT) and on.rec.tobytes() == twin.rec.tobytes()
    off = KLTTrackSequence(_tc(), frames, NFEAT, replace_lost=True, prefetch=prefetch)
    assert off.rec.tobytes() != on.rec.tobytes()


@pytest.mark.parametrize("sequential", [False, True], ids=["pingpong", "sequential"])
def test_toggling_between_calls_on_the_same_frame_objects(sequential):
    """one tracking context, the same two array objects in every call; the switch, then the tile grid, then the clip limit change
    between calls: the frame cache must not hand back pyramids built under other equalisation parameters (in sequential mode the kept
    pyramid stays what the previous call built, as it does for the twin)"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    frames = pair()
    tc, twin = _tc(sequentialMode=sequential), _tc(sequentialMode=sequential)
    settings = [(None, (8, 8), 3.0), ("clahe", (8, 8), 3.0), ("clahe", (8, 8), 3.0), ("clahe", (4, 5), 3.0), ("clahe", (4, 5), None),
                (None, (4, 5), None), ("clahe", (8, 8), 3.0)]
    for step, (switch, tiles, limit) in enumerate(settings):
        tc.equalization, tc.clahe_tiles, tc.clahe_clip_limit = switch, tiles, limit
        theirs = equalised(frames, tiles, limit) if switch else frames
        what = "step %d (%r, %r, %r)" % (step, switch, tiles, limit)
        if step % 2 == 0:                                      # a selection in every other step; the steps between track the list on
            fl, fl_twin = KLTSelectGoodFeatures(tc, frames[0], NFEAT), KLTSelectGoodFeatures(twin, theirs[0], NFEAT)
            _same(_records(fl), _records(fl_twin), what + ", selection")
        KLTTrackFeatures(tc, frames[0], frames[1], fl)
        KLTTrackFeatures(twin, theirs[0], theirs[1], fl_twin)
        _same(_records(fl), _records(fl_twin), what + ", tracking")


def test_frames_the_switch_takes():
    from PIL import Image
    from pyfeaturetrack_amd.selectGoodFeatures import KLTSelectGoodFeatures
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    frames = pair()
    tc = _tc(equalization="clahe")
    want = _records(KLTSelectGoodFeatures(_tc(), equalised(frames)[0], NFEAT))
    grey = [Image.fromarray(f, "L") for f in frames]
    fl = KLTSelectGoodFeatures(tc, grey[0], NFEAT)
    _same(_records(fl), want, "an 'L' image")
    KLTTrackFeatures(tc, grey[0], grey[1], fl)
    fl_twin = KLTSelectGoodFeatures(_tc(), equalised(frames)[0], NFEAT)
    KLTTrackFeatures(_tc(), equalised(frames)[0], equalised(frames)[1], fl_twin)
    _same(_records(fl), _records(fl_twin), "'L' images tracked")
    rgb = Image.fromarray(np.dstack([frames[0]] * 3), "RGB")
    for bad in (rgb, grey[0].convert("F"), frames[0].astype(np.float32), np.dstack([frames[0]] * 3)):
        with pytest.raises(ValueError, match="tc.equalization"):
            KLTSelectGoodFeatures(tc, bad, NFEAT)
        with pytest.raises(ValueError, match="tc.equalization"):
            KLTTrackFeatures(tc, frames[0], bad, fl)
        with pytest.raises(ValueError, match="tc.equalization"):
            KLTTrackSequence(tc, [frames[0], bad], NFEAT)
    small = _tc(equalization="clahe", clahe_tiles=(64, 64))
    with pytest.raises(ValueError, match="tc.equalization"):
        KLTSelectGoodFeatures(small, frames[0][:50, :200], NFEAT)
    # the refusals left nothing behind: the next call is the first one again
    _same(_records(KLTSelectGoodFeatures(tc, frames[0], NFEAT)), want, "after the refusals")


def test_equalize_image():
    from PIL import Image
    import pyfeaturetrack_amd as klt
    from pyfeaturetrack_amd.selectGoodFeatures import KLTEqualizeImage
    assert klt.KLTEqualizeImage is KLTEqualizeImage
    frames = pair()
    for tc, tiles, limit in ((_tc(), (8, 8), 3.0), (_tc(clahe_tiles=(3, 2), clahe_clip_limit=40.0), (3, 2), 40.0),
                             (_tc(equalization="clahe", clahe_tiles=(5, 7), clahe_clip_limit=None), (5, 7), None)):
        got = KLTEqualizeImage(tc, frames[0])
        want = equalised(frames, tiles, limit)[0]
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), (tiles, limit)
        assert KLTEqualizeImage(tc, Image.fromarray(frames[0], "L")).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="tc.equalization"):
        KLTEqualizeImage(_tc(), frames[0].astype(np.float32))
    with pytest.raises(ValueError, match="tc.equalization"):
        KLTEqualizeImage(_tc(clahe_tiles=(64, 64)), frames[0][:50])
