"""KLTTrackSequence with every post-track stage switched on, across the 64-row chunk edge of its record tables, against the per-frame loop
of the reference-shaped API on the same frames: the feature table and the three parallel tables (homography, crowd, quality) byte for
byte.  Rows 63 .. 66 of all four tables lie across the chunk edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCOLS, NROWS, NFRAMES, NFEAT = 160, 120, 67, 32


def _tc():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    tc = KLT_TrackingContext()
    tc.nPyramidLevels, tc.subsampling = 2, 4
    tc.KLTUpdateTCBorder()
    tc.sequentialMode = True
    tc.forwardBackwardCheck = tc.homographyCheck = tc.crowdingCheck = tc.trackQuality = True
    return tc


@pytest.fixture(scope="module")
def frames():
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(NCOLS, NROWS, 5)
    return [synth.synth_frame(NCOLS, NROWS, 5, k, base=base) for k in range(NFRAMES)]


@pytest.fixture(scope="module")
def quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    yield
    sgf.KLT_verbose, tf.KLT_verbose = old


@pytest.fixture(scope="module")
def loop(frames, quiet):
    """the per-frame loop, once: (lists, homography records, crowd records, quality records) per frame, None at frame 0"""
    from pyfeaturetrack_amd.selectGoodFeatures import KLTReplaceLostFeatures, KLTSelectGoodFeatures, features_to_array
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    tc = _tc()
    fl = KLTSelectGoodFeatures(tc, frames[0], NFEAT)
    lists, homography, crowd, quality = [features_to_array(fl)], [None], [None], [None]
    age = None
    for k in range(1, NFRAMES):
        KLTTrackFeatures(tc, frames[k - 1], frames[k], fl, age=age)
        homography.append(np.array(tc.homography_last))
        crowd.append(np.array(tc.crowding_last))
        quality.append(np.array(tc.quality_last))
        age = tc.crowding_last["age"]
        KLTReplaceLostFeatures(tc, frames[k], fl)
        lists.append(features_to_array(fl))
    return lists, homography, crowd, quality


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: got %r, want %r" % (what, got, want)


@pytest.mark.parametrize("prefetch", [True, False])
def test_track_sequence_tables_equal_the_per_frame_loop_across_the_chunk_edge(frames, quiet, loop, prefetch):
    from pyfeaturetrack_amd.backend import CROWD_DTYPE, HOMOGRAPHY_DTYPE, QUALITY_DTYPE
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    lists, homography, crowd, quality = loop
    ft = KLTTrackSequence(_tc(), frames, NFEAT, prefetch=prefetch)
    assert ft.rec.shape == ft.crowd.shape == ft.quality.shape == (NFRAMES, NFEAT) and ft.homography.shape == (NFRAMES,)
    assert ft.models is None and ft.epipolar is None
    for k in range(NFRAMES):
        _same(ft.rec[k], lists[k], "list of frame %d" % k)
        _same(ft.homography[k], homography[k] if k else np.zeros((), HOMOGRAPHY_DTYPE), "homography record of frame %d" % k)
        _same(ft.crowd[k], crowd[k] if k else np.zeros(NFEAT, CROWD_DTYPE), "crowd records of frame %d" % k)
        _same(ft.quality[k], quality[k] if k else np.zeros(NFEAT, QUALITY_DTYPE), "quality records of frame %d" % k)
    # the clip does what the stages are there for: features are lost and replaced on the way, and the records are no empty ones
    replaced = sum(int((lists[k]["val"] > 0).sum()) for k in range(1, NFRAMES))
    valid = sum(int(h["valid"] == 1) for h in homography[1:])
    print("replaced %d, valid homographies %d of %d, measured in the last rows %r" % (replaced, valid, NFRAMES - 1,
                                                                                     [int((q["val"] == 1).sum()) for q in quality[63:]]))
    assert replaced > 0 and valid >= NFRAMES // 2 and all((q["val"] == 1).any() for q in quality[63:])
