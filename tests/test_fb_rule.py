"""The forward-backward rule on the CPU oracle alone (no GPU), and the host-side pins of the feature."""
import numpy as np
import pytest

from fb_expected import KLT_FB_INCONSISTENT, KLT_TRACKED, OCCLUSION_CASES, fb_compose, occlusion_pair
from helpers import make_tc, params_from_tc


def oracle_tracker(ko, p, f0, f1):
    pyr = {1: ko.Pyramids(p, f0.astype(np.float32)), 2: ko.Pyramids(p, f1.astype(np.float32))}

    def track(fl, a, b):
        ko.track_features(p, pyr[a], pyr[b], fl)
        return fl
    return track


@pytest.mark.parametrize("case", OCCLUSION_CASES, ids=[c[0] for c in OCCLUSION_CASES])
def test_rule_on_the_occlusion_pairs(case):
    """Two oracle tracker runs and the rule on the occlusion pairs: the input is only meaningful if the check rejects some features the
    plain forward run calls tracked and keeps others.  Observed with max_error = 1.0 (recorded, not asserted):
        320x240_w7:   150 selected, 130 tracked forward, 19 rejected, 111 kept
        640x480_w15:  300 selected, 272 tracked forward, 17 rejected, 255 kept
        320x240_w9:   150 selected, 137 tracked forward, 20 rejected, 117 kept"""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, block, n = case
    assert levels >= 2
    f0, f1 = occlusion_pair(width, height, block)
    p = params_from_tc(make_tc(levels=levels, ss=ss, window=window))
    fin = ko.select_good_features(p, f0.astype(np.float32), n)
    out, fwd, back = fb_compose(oracle_tracker(ko, p, f0, f1), fin, 1.0)
    tracked = (fin["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
    rejected = tracked & (out["val"] == KLT_FB_INCONSISTENT)
    kept = tracked & (out["val"] == KLT_TRACKED)
    print("%s: %d selected, %d tracked forward, %d rejected, %d kept" % (name, int((fin["val"] >= 0).sum()), int(tracked.sum()),
                                                                        int(rejected.sum()), int(kept.sum())))
    assert rejected.any(), "no feature the forward run tracked is rejected: the pair does not exercise the check"
    assert kept.any(), "no feature is kept"
    assert np.array_equal(rejected | kept, tracked)
    # a kept feature is the forward record, a rejected one (-1, -1, KLT_FB_INCONSISTENT); everything else is the forward run's
    assert np.array_equal(out[~rejected], fwd[~rejected])
    assert (out["x"][rejected] == -1).all() and (out["y"][rejected] == -1).all()
    # with a limit nothing exceeds only features the backward run lost are rejected
    out_inf = fb_compose(oracle_tracker(ko, p, f0, f1), fin, 1e9)[0]
    assert np.array_equal(out_inf["val"] == KLT_FB_INCONSISTENT, tracked & (back["val"] != KLT_TRACKED))


def test_status_code_and_defaults():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState
    from pyfeaturetrack_amd.params import fb_params_from_tc
    assert kltState.KLT_FB_INCONSISTENT == -6
    tc = KLT_TrackingContext()
    assert tc.forwardBackwardCheck is False and tc.fb_max_error == 1.0
    f = fb_params_from_tc(tc)
    assert f.enabled == 0 and f.max_error == 1.0

    class Foreign:                       # a context made elsewhere has neither field
        affineConsistencyCheck = -1
    f = fb_params_from_tc(Foreign())
    assert f.enabled == 0 and f.max_error == 1.0


def test_both_checks_raise_before_any_device_work():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import fb_params_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    tc = KLT_TrackingContext()
    tc.forwardBackwardCheck = True
    tc.affineConsistencyCheck = 2
    img = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError, match="forwardBackwardCheck"):
        fb_params_from_tc(tc)
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        with pytest.raises(ValueError, match="forwardBackwardCheck"):
            KLTTrackFeatures(tc, img, img, [KLT_Feature() for _ in range(4)])
        with pytest.raises(ValueError, match="forwardBackwardCheck"):
            KLTTrackSequence(tc, [img, img], 4)
    finally:
        trk.KLT_verbose = verbose
    tc.affineConsistencyCheck = -1
    tc.fb_max_error = -0.5
    with pytest.raises(ValueError, match="fb_max_error"):
        fb_params_from_tc(tc)
    tc.fb_max_error = float("nan")
    with pytest.raises(ValueError, match="fb_max_error"):
        fb_params_from_tc(tc)


def test_print_tracking_context_unchanged(capsys):
    """KLTPrintTrackingContext prints the reference's lines and nothing about the check (what test_print_tracking_context pins)."""
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    KLTPrintTrackingContext(tc)
    plain = capsys.readouterr().out
    tc.forwardBackwardCheck, tc.fb_max_error = True, 0.25
    KLTPrintTrackingContext(tc)
    with_check = capsys.readouterr().out
    assert "\tborderx = 30.0\n" in plain and "\tnPyramidLevels = 2\n" in plain and "\tmax_residue = None\n" in plain
    assert "forwardBackward" not in plain and "fb_max_error" not in plain
    names = [line.split(" = ")[0].strip() for line in plain.splitlines() if " = " in line]
    assert names == ["mindist", "window_width", "window_height", "sequentialMode", "smoothBeforeSelecting", "writeInternalImages",
                     "min_eigenvalue", "min_determinant", "min_displacement", "max_iterations", "max_residue", "grad_sigma",
                     "smooth_sigma_fact", "pyramid_sigma_fact", "nSkippedPixels", "borderx", "bordery", "nPyramidLevels", "subsampling",
                     "pyramid_last", "pyramid_last_gradx", "pyramid_last_grady"]
    assert plain.split("\n", 1)[1] == with_check.split("\n", 1)[1]          # (the first line is the object's repr)


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi
    import ctypes
    for name in ("klt_set_fb_params", "klt_track_fb_async", "klt_track_fb", "klt_track_fb_batch_async"):
        assert name in _abi.SYMBOLS
    assert ctypes.sizeof(_abi.KltFbParams) == 8
    lib = ctypes.CDLL(_abi.LIB_PATH)
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11 and hasattr(lib, "klt_track_fb_batch_async")
