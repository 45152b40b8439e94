"""The track-quality rule on the CPU (no GPU): the numpy restatement of tests/quality_expected.py against the CPU oracle's residue test, on
a lighting change, on every kind of record it does not measure -- and the host layer: the ABI's declarations and the order in which
KLTTrackSequence enqueues the quality launches."""
import ctypes

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from light_expected import LIT_SHIFT
from quality_expected import (KLT_LARGE_RESIDUE, KLT_TRACKED, QUALITY_DTYPE, edge_positions, measured, quality_expected, quality_record,
                              records, shifted_case, unmeasured_kinds)

def test_identical_frames_give_residue_zero_and_ncc_one():
    """out = in on one frame: T_k == S_k, so every |T_k - S_k| is 0 and a == b == c bit for bit (the same operations on the same
    numbers); sqrt(a*a) == a exactly (the correctly rounded root of a square that did not overflow), and c / a == 1"""
    from oracle import klt_oracle as ko
    c = shifted_case()
    fin = c["fin"]
    out = fin.copy()
    out["val"] = KLT_TRACKED
    q = quality_expected(ko, c["pyr1"], c["pyr1"], fin, out, 7)
    assert (q["val"] == 1).all()
    assert (q["residue"] == 0).all()
    assert (q["ncc"] == np.float32(1.0)).all(), q["ncc"].min()
    assert (q["min_eig"] > 0).all()
    fin = fin.copy()                                    # ... and at positions off the pixel grid
    fin["x"] += np.float32(0.37)
    fin["y"] -= np.float32(0.61)
    out = fin.copy()
    out["val"] = KLT_TRACKED
    q = quality_expected(ko, c["pyr1"], c["pyr1"], fin, out, 7)
    assert (q["val"] == 1).all() and (q["residue"] == 0).all() and (q["ncc"] == np.float32(1.0)).all()


def test_residue_is_the_number_max_residue_tests():
    """The oracle's tracker without max_residue, then with max_residue = r, the median measured residue of the tracked features: a
    feature tracked in the first run is KLT_LARGE_RESIDUE in the second iff its measured residue > float32(r), else KLT_TRACKED."""
    from oracle import klt_oracle as ko
    c = shifted_case()
    fin = c["fin"]
    first = fin.copy()
    ko.track_features(c["p"], c["pyr1"], c["pyr2"], first)
    q = quality_expected(ko, c["pyr1"], c["pyr2"], fin, first, 7)
    tracked = first["val"] == KLT_TRACKED
    assert tracked.sum() >= 200 and np.array_equal(q["val"] == 1, tracked)
    r = np.float32(np.median(q["residue"][tracked]))
    p = params_from_tc(make_tc(levels=2, ss=4, window=7, max_residue=float(r)))
    assert np.float32(p.max_residue) == r
    second = fin.copy()
    ko.track_features(p, c["pyr1"], c["pyr2"], second)
    large = q["residue"] > r
    print("tracked %d, median residue %r, above it %d" % (tracked.sum(), r, (large & tracked).sum()))
    assert (large & tracked).sum() >= 50 and (~large & tracked).sum() >= 50          # both sides of the median are populated
    assert np.array_equal(second["val"][tracked & large], np.full((tracked & large).sum(), KLT_LARGE_RESIDUE))
    assert np.array_equal(second["val"][tracked & ~large], np.full((tracked & ~large).sum(), KLT_TRACKED))
    assert np.array_equal(second["x"][tracked & ~large], first["x"][tracked & ~large])


def test_a_lighting_change_explodes_the_residue_and_leaves_the_ncc():
    """out = in + LIT_SHIFT as given positions on the pair without a lighting change and on the lit pair (gain 0.5, offset 40).
    Measured on this restatement: see the figures beside the assertions."""
    from oracle import klt_oracle as ko
    c = shifted_case()
    fin = c["fin"]
    out = records(fin["x"] + np.float32(LIT_SHIFT[0]), fin["y"] + np.float32(LIT_SHIFT[1]))
    plain = quality_expected(ko, c["pyr1"], c["pyr2"], fin, out, 7)
    lit = quality_expected(ko, c["pyr1"], c["pyr2_lit"], fin, out, 7)
    assert (plain["val"] == 1).all() and (lit["val"] == 1).all()                 # all 300 features are measured
    d = np.abs(lit["ncc"] - plain["ncc"])
    print("residue median plain %.4f lit %.4f (min lit %.4f); ncc median plain %.6f lit %.6f; |ncc lit - ncc plain| median %.6f max %.6f; "
          "min_eig ratio median %.4f"
          % (np.median(plain["residue"]), np.median(lit["residue"]), lit["residue"].min(), np.median(plain["ncc"]), np.median(lit["ncc"]),
             np.median(d), d.max(), np.median(lit["min_eig"] / plain["min_eig"])))
    # measured: residue median 1.5577 without the change, 21.5447 with it (smallest 6.3648) -- |T - (0.5 T + 40)| = |0.5 T - 40| is some
    # 24 grey levels for a mid-grey window -- against the customary max_residue of 10
    assert np.median(lit["residue"]) > 10.0 and np.median(lit["residue"]) > 5.0 * np.median(plain["residue"])
    assert np.median(plain["residue"]) < 3.0
    # measured: ncc median 0.999127 on both pairs; |ncc lit - ncc plain| median 0.000057, maximum 0.000931.  The margin is frame 2's u8
    # rounding: 0.5 m + 40 of an odd m is rounded up by 0.5, a pattern of variance 1/16 on a window whose contrast the gain has halved.
    # For a window of standard deviation sT it lowers the ncc by about (1/16) / (2 * 0.25 sT^2) and moves the cross term by about
    # 0.25 / (0.5 sT) / sqrt(49): 0.005 + 0.014 < 0.02 at sT = 5 grey levels, far below what the selection picks
    assert abs(np.median(lit["ncc"]) - np.median(plain["ncc"])) < 1e-3
    assert np.median(d) < 1e-3 and d.max() < 0.02
    assert np.median(lit["ncc"]) > 0.99
    # the gradients of frame 2 carry the gain squared: measured median ratio 0.2502
    assert 0.2 < np.median(lit["min_eig"] / plain["min_eig"]) < 0.3


def _planes(ncols=64, nrows=48, seed=3):
    """level-0 planes made directly (the rule only samples them): a smooth random image and two gradient planes"""
    rs = np.random.RandomState(seed)
    img = rs.uniform(0.0, 255.0, (nrows, ncols)).astype(np.float32)
    return img, rs.uniform(-30.0, 30.0, (nrows, ncols)).astype(np.float32), rs.uniform(-30.0, 30.0, (nrows, ncols)).astype(np.float32)


@pytest.mark.parametrize("w", [3, 7, 15, 31])
def test_records_that_are_not_measured_are_all_zero(w):
    """a lost `in`, every loss code in `out`, out.val > 0, NaN / +-inf / 1e30 / negative / == ncols coordinates on either side, windows that
    touch each of the four edges on either side (the first position outside: all zero; the last one inside: measured)"""
    from oracle import klt_oracle as ko
    ncols, nrows = 64, 48
    img, gx, gy = _planes(ncols, nrows)
    fin = records(np.full(120, ncols // 2 + 0.5), np.full(120, nrows // 2 + 0.25), 1)
    fout = records(np.full(120, ncols // 2 + 0.5), np.full(120, nrows // 2 + 0.25), KLT_TRACKED)
    fin, fout, want = unmeasured_kinds(fin, fout, w, ncols, nrows)
    assert sum(want.values()) >= 18 and len(want) - sum(want.values()) >= 60
    for i, is_measured in want.items():
        q = quality_record(ko, img, img, gx, gy, fin[i], fout[i], w)
        assert measured(fin[i], fout[i], w, ncols, nrows) == is_measured, (i, fin[i], fout[i])
        if is_measured:
            assert q[3] == 1 and q[2] > 0, (i, fin[i], fout[i], q)
        else:
            assert q == (0, 0, 0, 0), (i, fin[i], fout[i], q)
    # the last position inside reads the frame's last row and column, the first one outside would read behind them
    for x, y, fits in edge_positions(w, ncols, nrows):
        ix, iy, hw = int(x), int(y), w // 2
        assert fits == (ix - hw >= 0 and iy - hw >= 0 and ix + hw + 1 <= ncols - 1 and iy + hw + 1 <= nrows - 1)


def test_a_constant_region():
    """constant image, no gradient: residue 0, a == b == 0 exactly (49 * 49 v^2 - (49 v)^2 with v = 100, every product exact), so ncc 0;
    min_eig 0; the record is measured"""
    from oracle import klt_oracle as ko
    img = np.full((48, 64), 100.0, np.float32)
    zero = np.zeros_like(img)
    fin = records([20.25, 30.0], [20.5, 17.0], 3)
    fout = records([24.75, 31.0], [19.5, 18.0])
    for i in range(2):
        q = quality_record(ko, img, img, zero, zero, fin[i], fout[i], 7)
        assert q == (0, 0, 0, 1), q
        assert all(np.signbit(v) == 0 for v in q[:3])


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi, backend
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_track_quality_async", "klt_track_quality_batch_async", "klt_track_quality"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_abi.KltQuality) == 16 == ctypes.sizeof(_abi.KltFeat)
    assert ctypes.alignment(_abi.KltQuality) == ctypes.alignment(_abi.KltFeat)
    assert backend.QUALITY_DTYPE == QUALITY_DTYPE and backend.QUALITY_DTYPE.itemsize == 16
    assert [backend.QUALITY_DTYPE.fields[k][1] for k in ("residue", "ncc", "min_eig", "val")] == [0, 4, 8, 12]
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11


def test_tracking_context_switch_is_off_and_silent(capsys):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    assert tc.trackQuality is False
    KLTPrintTrackingContext(tc)
    assert "trackQuality" not in capsys.readouterr().out


@pytest.mark.timeout(60)
@pytest.mark.parametrize("nframes", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("on", [False, True])
def test_track_sequence_enqueues_quality_behind_every_tracker(nframes, on):
    """KLTTrackSequence's host logic on the recording context of tests/test_host_and_abi.py: without tc.trackQuality no quality launch;
    with it one behind every tracker launch -- a repeated one included (the recorder's select_finish reports a rewritten list now and
    then) --, directly behind it, on the same slots and rows, into the row of the quality table that stands for the tracker's output row"""
    from test_host_and_abi import _recording_context
    from pyfeaturetrack_amd import trackSequence as ts
    from pyfeaturetrack_amd.klt import KLT_TrackingContext

    h, w, n = 48, 64, 10
    frames = [np.full((h, w), k, np.uint8) for k in range(nframes)]
    tc = KLT_TrackingContext()
    tc.sequentialMode = False
    if on:
        tc.trackQuality = True
    else:
        del tc.__dict__["trackQuality"]                      # a context made elsewhere has no such field: read with a default
    ctx = _recording_context()

    def track_quality_async(s1, s2, fb_in, fb_out, fb_quality, count):
        ctx.log.append(("quality", ctx.frame_in_slot[s1], ctx.frame_in_slot[s2], fb_in, fb_out, fb_quality, count))
    ctx.track_quality_async = track_quality_async
    tc.__dict__["_klt_ctx"] = ctx
    ft = ts._track_sequence_locked(ctx, tc, iter(frames), n, True, True, True)
    assert ft.nFrames == nframes
    log = ctx.log
    quality = [i for i, e in enumerate(log) if e[0] == "quality"]
    trackers = [i for i, e in enumerate(log) if e[0] == "track"]
    if not on:
        assert not quality and ft.quality is None
        return
    assert len(trackers) >= nframes - 1 and len(quality) == len(trackers)
    if nframes >= 4:
        assert len(trackers) > nframes - 1, "the recorder repeats a tracker now and then"
    for i in trackers:
        t, q = log[i], log[i + 1]
        assert q[0] == "quality" and q[1:5] == t[1:5] and q[6] == n, (t, q)           # the same frames and rows, directly behind
        assert q[5] - ts._FBQ_TABLE == t[4] - ts._FB_TABLE                             # the quality row of the tracker's output row
        replace = [k for k, e in enumerate(log) if e[0] == "replace" and e[1] == t[2]]
        assert replace and i + 1 < replace[0]                                          # in front of that frame's replacement
    assert ft.quality.shape == (nframes, n) and ft.quality.dtype == QUALITY_DTYPE
    assert (ft.quality["val"][0] == 0).all() and (ft.quality["residue"][0] == 0).all()
