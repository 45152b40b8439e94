"""The gain / bias tracking rule on the CPU (no GPU): the numpy restatement of tests/light_expected.py against the CPU oracle's plain
tracker, the degenerate-window rule, and the host layer's switch (params.light_params_from_tc, the ABI's two entry points)."""
import ctypes

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from light_expected import (KLT_LARGE_RESIDUE, KLT_SMALL_DET, KLT_TRACKED, LIT_SHIFT, ZERO_RECT, light_case, light_track, lit_pair, shares)


def test_lit_pair_is_kept_by_the_rule_and_lost_by_the_plain_tracker():
    """320x240, 300 features selected on frame 1, frame 2 = 0.5 * (frame 1 moved by (1.3, -0.8)) + 40, max_residue = 10, 7x7, 2 levels,
    subsampling 4.  Measured: the rule keeps 230 of 300 (57 lost to KLT_LARGE_RESIDUE, 13 out of bounds), the oracle's plain tracker 12 of
    300 (223 lost to KLT_LARGE_RESIDUE): a ratio of 19.  Position error of the kept features against the true shift: median 0.436 px,
    maximum 1.645 px -- the text of KLT 1.3.4 matches mean and energy of the two windows, not their contrast (alpha = 1.23 where the gain
    is 2), so a residual of the template's own structure stays and biases the minimum.  (With gain 0.7 the same pair measured 267 against
    207 kept, a ratio of 1.3: there the plain difference 0.3 T - 40 is small for mid-grey windows.)"""
    from oracle import klt_oracle as ko
    c = light_case(320, 240, 7, 2, 4, n=300, edge=False, max_residue=10.0)
    fin, want = c["fin"], c["want"]
    plain = fin.copy()
    ko.track_features(c["p"], c["pyr1"], c["pyr2"], plain)
    kept, live = shares(fin, want)
    plain_kept, _ = shares(fin, plain)
    k = want["val"] == KLT_TRACKED
    err = np.hypot(want["x"][k] - fin["x"][k] - LIT_SHIFT[0], want["y"][k] - fin["y"][k] - LIT_SHIFT[1])
    print("rule keeps %d of %d, plain tracker %d (%d large residue); error median %.3f max %.3f px"
          % (kept, live, plain_kept, (plain["val"] == KLT_LARGE_RESIDUE).sum(), np.median(err), err.max()))
    assert live == 300
    assert kept >= 0.7 * live                       # measured 0.767
    assert plain_kept <= 0.1 * live                 # measured 0.04
    assert (plain["val"] == KLT_LARGE_RESIDUE).sum() >= 0.6 * live      # measured 0.743
    assert kept >= 2 * plain_kept
    assert np.median(err) < 0.6 and err.max() < 2.0                     # measured 0.436 / 1.645
    assert not np.isnan(want["x"]).any() and not np.isnan(want["y"]).any()


def test_gain_one_offset_zero_is_the_plain_tracker():
    """Gain 1, offset 0.  On identical frames alpha = alpha_g = 1 and beta = 0 exactly: the rule's records are the plain oracle's bit for
    bit.  On a moved frame the two trackers agree to 1e-2 px where both have CONVERGED to a common minimum -- a whole-pixel shift (2, -1)
    (the periodic texture rolled: at the true position both differences vanish), min_displacement 1e-4 and 100 iterations (a tracker stops
    within a few thresholds of its minimum, so the threshold has to be far below the bound): measured 0.0032 px over the 276 features both
    keep.  With the default threshold 0.1 the same pair differs by up to 0.43 px (median 0.036), and with a sub-pixel shift (1.3, -0.8)
    and converged trackers by up to 0.21 px (median 0.038): there the windows differ by the resampling, alpha is not 1, and the two
    objectives have different minima."""
    from oracle import klt_oracle as ko
    tc = make_tc(levels=2, ss=4, window=7, max_residue=10.0)
    p = params_from_tc(tc)
    f1, _ = lit_pair(320, 240, gain=1.0, offset=0.0)
    fin = ko.select_good_features(p, f1.astype(np.float32), 300)
    fin["val"][4::31] = -3
    pyr1 = ko.Pyramids(p, f1.astype(np.float32))
    plain = fin.copy()
    ko.track_features(p, pyr1, pyr1, plain)
    same = light_track(p, pyr1, pyr1, fin)
    for name in ("x", "y", "val"):
        assert np.array_equal(same[name], plain[name]), name

    tc = make_tc(levels=2, ss=4, window=7, max_residue=10.0, min_displacement=1e-4, max_iterations=100)
    p = params_from_tc(tc)
    f1, f2 = lit_pair(320, 240, shift=(2.0, -1.0), gain=1.0, offset=0.0)
    pyr1, pyr2 = ko.Pyramids(p, f1.astype(np.float32)), ko.Pyramids(p, f2.astype(np.float32))
    plain = fin.copy()
    ko.track_features(p, pyr1, pyr2, plain)
    got = light_track(p, pyr1, pyr2, fin)
    both = (fin["val"] >= 0) & (got["val"] == KLT_TRACKED) & (plain["val"] == KLT_TRACKED)
    d = np.maximum(np.abs(got["x"][both] - plain["x"][both]), np.abs(got["y"][both] - plain["y"][both]))
    print("both keep %d, largest difference %.4f px" % (both.sum(), d.max()))
    assert both.sum() >= 250                        # measured 276 (286 of the full list, before ten slots were marked lost)
    assert d.max() <= 1e-2


def test_all_zero_window_ends_small_det_and_nothing_is_nan():
    """the edge pair (a rectangle of frame 2 set to zero): a feature whose frame-2 windows are all zero ends KLT_SMALL_DET with position
    (-1, -1); no record of any case holds a NaN, whatever the window and with or without the residue test"""
    for window in (7, 15, 5):
        for mr in (None, 10.0):
            c = light_case(window=window, max_residue=mr)
            fin, want = c["fin"], c["want"]
            assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()
            x0, y0, x1, y1 = ZERO_RECT
            m = 3 * (window // 2) + 8               # the coarse level's window (twice as wide in level-0 pixels) and the smoothing's reach
            deep = (fin["val"] >= 0) & (fin["x"] > x0 + m) & (fin["x"] < x1 - m) & (fin["y"] > y0 + m) & (fin["y"] < y1 - m)
            if window <= 7:
                assert deep.sum() >= 3, deep.sum()
            assert (want["val"][deep] == KLT_SMALL_DET).all()
            assert (want["x"][deep] == -1.0).all() and (want["y"][deep] == -1.0).all()
            dead = fin["val"] < 0
            for name in ("x", "y", "val", "aux"):
                assert np.array_equal(want[name][dead], fin[name][dead])        # a slot that is not live passes through


def test_degenerate_sums_on_the_bits():
    """light_gain: zero, negative, infinite and NaN sums, and quotients whose root is not finite, are refused; nothing non-finite comes
    out of a refused window's gain (the sums count as 1)"""
    from light_expected import light_gain
    f = np.float32
    nf = f(49.0)
    good = np.array([100.0], f)
    for bad in (0.0, -0.0, -3.0, np.inf, np.nan):
        for slot in range(4):
            sums = [good.copy() for _ in range(4)]
            sums[slot][0] = bad
            ok, alpha, beta, alpha_g = light_gain(sums[0], sums[1], sums[2], sums[3], nf)
            assert not ok[0] and alpha[0] == 1.0 and beta[0] == 0.0 and alpha_g[0] == 1.0
    ok, alpha, _, _ = light_gain(good, np.array([3e38], f), good, np.array([1e-45], f), nf)     # sq1 / sq2 overflows: alpha = inf
    assert not ok[0] and np.isinf(alpha[0])
    ok, alpha, beta, alpha_g = light_gain(np.array([98.0], f), np.array([4 * 49.0], f), np.array([49.0], f), np.array([49.0], f), nf)
    assert ok[0] and alpha[0] == 2.0 and beta[0] == 0.0 and alpha_g[0] == f(np.sqrt(2.0))


def test_light_params_from_tc():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import light_params_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    tc = KLT_TrackingContext()
    assert tc.lightingCompensation is None and light_params_from_tc(tc).mode == 0

    class Foreign:                       # a context made elsewhere has no such field
        affineConsistencyCheck = -1
    assert light_params_from_tc(Foreign()).mode == 0
    tc.lightingCompensation = "gain_bias"
    assert light_params_from_tc(tc).mode == 1
    for bad in ("gain", "bias", True, 1, 0, ""):
        tc.lightingCompensation = bad
        with pytest.raises(ValueError, match="lightingCompensation"):
            light_params_from_tc(tc)
    tc.lightingCompensation = "gain_bias"
    for attr, on, off in (("forwardBackwardCheck", True, False), ("motionPrediction", "constant_velocity", None), ("affineConsistencyCheck", 0, -1),
                          ("affineConsistencyCheck", 2, -1)):
        setattr(tc, attr, on)
        with pytest.raises(ValueError, match="lightingCompensation"):
            light_params_from_tc(tc)
        setattr(tc, attr, off)
    with pytest.raises(ValueError, match="lightingCompensation"):
        light_params_from_tc(tc, guess=True)
    with pytest.raises(ValueError, match="lightingCompensation"):
        light_params_from_tc(tc, sequence=True)
    assert light_params_from_tc(tc).mode == 1
    # ... and through the entry points, before any device work (this machine may have no device at all)
    img = np.zeros((64, 64), np.uint8)
    fl = [KLT_Feature() for _ in range(4)]
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        with pytest.raises(ValueError, match="lightingCompensation"):
            KLTTrackSequence(tc, [img, img], 4)
        with pytest.raises(ValueError, match="lightingCompensation"):
            KLTTrackFeatures(tc, img, img, fl, guess=np.zeros((4, 2), np.float32))
        tc.forwardBackwardCheck = True
        with pytest.raises(ValueError, match="lightingCompensation"):
            KLTTrackFeatures(tc, img, img, fl)
        tc.forwardBackwardCheck = False
        tc.lightingCompensation = "both"
        with pytest.raises(ValueError, match="lightingCompensation"):
            KLTTrackFeatures(tc, img, img, fl)
    finally:
        trk.KLT_verbose = verbose
    # the reference's own switch raises as the reference does
    tc = KLT_TrackingContext()
    tc.lighting_insensitive = True
    with pytest.raises(Exception, match="Not implemented"):
        params_from_tc(tc)
    tc.lightingCompensation = "gain_bias"
    with pytest.raises(Exception, match="Not implemented"):
        params_from_tc(tc)


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_set_light_params", "klt_track_light_path"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_abi.KltLightParams) == 4
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11
