"""The motion-prior rule on the CPU oracle alone (no GPU), and the host-side pins of the feature."""
import numpy as np
import pytest

from fb_expected import OCCLUSION_CASES, occlusion_pair
from guess_expected import (KLT_OOB, KLT_TRACKED, LARGE_SHIFT_CASES, guess_compose, guess_records, large_shift_pair, noisy_truth,
                            predict_cv, well_inside)
from helpers import make_tc, params_from_tc, synth251_frames


def _pyramids(ko, p, f0, f1):
    return ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))


def _identity_cases(img0, img1):
    yield "cfg-1", img0, img1, make_tc(max_residue=10.0), 100, 0
    frames = synth251_frames()
    yield "synth251", frames[0], frames[2], make_tc(), 80, 9
    for name, width, height, window, levels, ss, block, n in OCCLUSION_CASES:
        f0, f1 = occlusion_pair(width, height, block)
        yield name, f0, f1, make_tc(levels=levels, ss=ss, window=window), n, 13


def test_identity_and_invalid_guesses_are_the_plain_tracker(img0, img1):
    """the composition with every guess the feature's own position, with all guesses invalid (val < 0, NaN, infinities) and with no guess
    list equals ko.track_features byte for byte (x, y, val; the oracle writes no aux word, its iteration counts are compared instead)"""
    from oracle import klt_oracle as ko
    for name, f0, f1, tc, n, lost_every in _identity_cases(img0, img1):
        p = params_from_tc(tc)
        fin = ko.select_good_features(p, f0.astype(np.float32), n)
        if lost_every:
            fin["val"][3::lost_every] = -3
        pyr1, pyr2 = _pyramids(ko, p, f0, f1)
        want = fin.copy()
        _, want_it = ko.track_features(p, pyr1, pyr2, want, want_iters=True)
        own = guess_records(np.stack([fin["x"], fin["y"]], axis=1))
        invalid = own.copy()
        invalid["x"] += 25.0
        invalid["val"][0::3] = -1
        invalid["x"][1::3] = np.nan
        invalid["y"][2::3] = np.inf
        invalid["x"][5::6] = -np.inf
        for what, guess in (("identity", own), ("invalid", invalid), ("none", None)):
            got, it = guess_compose(ko, p, pyr1, pyr2, fin, guess, want_iters=True)
            for field in ("x", "y", "val"):
                assert got[field].tobytes() == want[field].tobytes(), (name, what, field)
            assert np.array_equal(it, want_it), (name, what)


@pytest.mark.parametrize("case", LARGE_SHIFT_CASES, ids=[c[0] for c in LARGE_SHIFT_CASES])
def test_large_shift_known_answer(case):
    """Frame 2 is the texture moved far beyond the search range; the guess is the true position plus uniform noise in [-2, 2] px.  Every
    feature whose true target lies more than 2 px inside the border is tracked to within 0.5 px of the truth; the plain tracker brings at
    most a tenth of them that close.  Measured (recorded, not asserted): 94 of 94 within 0.14 px (320x240_w7), 66 of 66 within 0.12 px
    (251x187_w7), 66 of 66 within 0.073 px (320x240_w15), 99 of 99 within 0.11 px (320x240_w9); the plain tracker: none in any case."""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, shift, n = case
    p = params_from_tc(make_tc(levels=levels, ss=ss, window=window))
    f0, f1 = large_shift_pair(width, height, shift)
    fin = ko.select_good_features(p, f0.astype(np.float32), n)
    pyr1, pyr2 = _pyramids(ko, p, f0, f1)
    guess, truth = noisy_truth(fin, shift)
    inside = well_inside(truth, p, width, height)
    assert inside.sum() >= 50, "the case has too few features whose target stays inside the image"
    out = guess_compose(ko, p, pyr1, pyr2, fin, guess)
    err = np.hypot(out["x"] - truth[:, 0], out["y"] - truth[:, 1])
    plain = fin.copy()
    ko.track_features(p, pyr1, pyr2, plain)
    plain_close = (plain["val"] == KLT_TRACKED) & (np.hypot(plain["x"] - truth[:, 0], plain["y"] - truth[:, 1]) < 0.5)
    print("%s: %d inside, %d tracked with the prior, max error %.3f px; plain tracker within 0.5 px: %d" % (
        name, inside.sum(), (out["val"][inside] == KLT_TRACKED).sum(), err[inside & (out["val"] == KLT_TRACKED)].max(),
        plain_close[inside].sum()))
    assert (out["val"][inside] == KLT_TRACKED).all()
    assert (err[inside] < 0.5).all()
    assert plain_close[inside].sum() <= inside.sum() // 10


def test_off_image_guesses_are_out_of_bounds():
    """a finite guess outside the image is caught by the first level's bounds test: KLT_OOB with that level alone in the aux word"""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, shift, n = LARGE_SHIFT_CASES[0]
    p = params_from_tc(make_tc(levels=levels, ss=ss, window=window))
    f0, f1 = large_shift_pair(width, height, shift)
    fin = ko.select_good_features(p, f0.astype(np.float32), 40)
    pyr1, pyr2 = _pyramids(ko, p, f0, f1)
    pos = np.stack([fin["x"], fin["y"]], axis=1).astype(np.float32)
    for k, (gx, gy) in enumerate(((1e30, 10.0), (-1e30, 10.0), (10.0, -5.0), (width + 0.5, 100.0), (100.0, height + 3.0), (-0.25, 50.0))):
        pos[k] = (gx, gy)
    out = guess_compose(ko, p, pyr1, pyr2, fin, guess_records(pos))
    for k in range(6):
        assert tuple(out[k]) == (-1.0, -1.0, KLT_OOB, 1 << (4 * (levels - 1))), (k, out[k])


def test_predictor_rule():
    from pyfeaturetrack_amd.klt import KLT_Feature
    from pyfeaturetrack_amd.trackFeatures import KLTPredictConstantVelocity
    from guess_expected import FEAT_DTYPE
    rs = np.random.RandomState(5)
    n = 64
    prev, cur = np.zeros(n, FEAT_DTYPE), np.zeros(n, FEAT_DTYPE)
    for a in (prev, cur):
        a["x"], a["y"] = rs.uniform(0, 300, n), rs.uniform(0, 200, n)
    prev["val"][::5] = 1234                                 # selected or replaced on the frame before: live, a position to move from
    prev["val"][1::7] = -4                                  # was lost before the step (then cur is lost too -- or was refilled)
    cur["val"][1::7] = 977
    cur["val"][2::9] = -2                                   # lost in the step
    cur["x"][2::9] = cur["y"][2::9] = -1.0
    cur["val"][3::11] = 4321                                # refilled by the replacement pass: no velocity
    g = predict_cv(prev, cur)
    ok = (cur["val"] == 0) & (prev["val"] >= 0)
    assert ok.any() and (~ok).any()
    assert (g["val"][ok] == 0).all() and (g["aux"] == 0).all()
    assert np.array_equal(g["x"][ok], (cur["x"] + (cur["x"] - prev["x"]))[ok]) and g["x"].dtype == np.float32
    assert np.array_equal(g["y"][ok], (cur["y"] + (cur["y"] - prev["y"]))[ok])
    assert (g["x"][~ok] == -1).all() and (g["y"][~ok] == -1).all() and (g["val"][~ok] == -1).all()
    # the host function: the same positions, NaN rows where there is no guess; record arrays, feature lists and plain positions
    got = KLTPredictConstantVelocity(prev, cur)
    assert got.dtype == np.float32 and got.shape == (n, 2)
    assert np.array_equal(got[ok, 0], g["x"][ok]) and np.array_equal(got[ok, 1], g["y"][ok]) and np.isnan(got[~ok]).all()

    def as_list(rec):
        fl = [KLT_Feature() for _ in range(len(rec))]
        for f, r in zip(fl, rec):
            f.x, f.y, f.val = float(r["x"]), float(r["y"]), int(r["val"])
        return fl
    assert np.array_equal(KLTPredictConstantVelocity(as_list(prev), as_list(cur)), got, equal_nan=True)
    positions = np.stack([prev["x"], prev["y"]], axis=1)
    positions[prev["val"] < 0] = np.nan
    assert np.array_equal(KLTPredictConstantVelocity(positions, as_list(cur)), got, equal_nan=True)


def test_defaults_and_value_errors_before_any_device_work():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import guess_records as api_guess_records, motion_prediction_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    tc = KLT_TrackingContext()
    assert tc.motionPrediction is None and motion_prediction_from_tc(tc) is None

    class Foreign:                       # a context made elsewhere has no such field
        affineConsistencyCheck = -1
    assert motion_prediction_from_tc(Foreign()) is None
    img = np.zeros((64, 64), np.uint8)
    fl = [KLT_Feature() for _ in range(4)]
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        tc.motionPrediction = "constant_velocity"
        assert motion_prediction_from_tc(tc) == "constant_velocity"
        for bad in ("linear", True, 1):
            tc.motionPrediction = bad
            with pytest.raises(ValueError, match="motionPrediction"):
                KLTTrackSequence(tc, [img, img], 4)
        tc.motionPrediction = "constant_velocity"
        tc.affineConsistencyCheck = 2
        with pytest.raises(ValueError, match="motionPrediction"):
            KLTTrackSequence(tc, [img, img], 4)
        tc.motionPrediction = None
        with pytest.raises(ValueError, match="guess"):
            KLTTrackFeatures(tc, img, img, fl, guess=np.zeros((4, 2), np.float32))
        tc.affineConsistencyCheck = -1
        for bad in (np.zeros((3, 2)), np.zeros((4, 3)), np.zeros(8)):
            with pytest.raises(ValueError, match="guess"):
                KLTTrackFeatures(tc, img, img, fl, guess=bad)
    finally:
        trk.KLT_verbose = verbose
    rec = api_guess_records([[1.5, 2.5], [np.nan, 3.0], [4.0, np.inf], [7.0, 8.0]], 4)
    assert rec["val"].tolist() == [0, -1, 0, 0] and rec["x"][0] == 1.5 and rec["y"][3] == 8.0 and np.isinf(rec["y"][2])
    assert api_guess_records(None, 4) is None


def test_print_tracking_context_says_nothing_of_the_prior(capsys):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    KLTPrintTrackingContext(tc)
    plain = capsys.readouterr().out
    tc.motionPrediction = "constant_velocity"
    KLTPrintTrackingContext(tc)
    with_prior = capsys.readouterr().out
    assert "motionPrediction" not in plain and plain.split("\n", 1)[1] == with_prior.split("\n", 1)[1]


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi
    import ctypes
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_track_guess_async", "klt_track_guess", "klt_track_guess_batch_async", "klt_track_fb_guess_async",
                 "klt_predict_cv_async"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11


def test_compat_names_take_the_keyword():
    import inspect
    import os
    import subprocess
    import sys
    from pyfeaturetrack_amd import trackFeatures
    assert "guess" in inspect.signature(trackFeatures.KLTTrackFeatures).parameters
    compat = os.path.join(os.path.dirname(os.path.abspath(trackFeatures.__file__)), "compat")
    code = ("import inspect, trackFeatures, klt; assert 'guess' in inspect.signature(trackFeatures.KLTTrackFeatures).parameters; "
            "assert hasattr(trackFeatures, 'KLTPredictConstantVelocity'); assert klt.KLT_TrackingContext().motionPrediction is None")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([compat, os.path.dirname(os.path.dirname(compat))]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env)
