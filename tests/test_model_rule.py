"""The motion-model rule on the CPU (no GPU): the numpy restatement of tests/model_expected.py on the moving-block pairs (lists from the
CPU oracle's selector and tracker), on synthetic lists with a known answer, on every way to end without a model and on every kind of
record that is not a candidate -- and the host layer: parameters, status code, ValueErrors, the ABI's declarations."""
import ctypes

import numpy as np
import pytest

from fb_expected import OCCLUSION_CASES, fb_compose
from helpers import make_tc, params_from_tc
from model_expected import (BLOCK_MOTION, FEAT_DTYPE, KLT_MODEL_OUTLIER, KLT_TRACKED, MODEL_DTYPE, block_sides, candidate_mask, mix,
                            model_affine, motion_check_expected, moving_block_pair, mulhi32, non_candidate_kinds, picks, records,
                            synthetic_lists)
from test_fb_rule import oracle_tracker


@pytest.mark.parametrize("case", OCCLUSION_CASES[:2], ids=[c[0] for c in OCCLUSION_CASES[:2]])
def test_the_moving_block_is_flagged_and_the_background_is_not(case):
    """A block whose texture moves by BLOCK_MOTION on a background that moves by (1.3, -0.8): the features on the block track perfectly
    well, pass the forward-backward check, and are wrong for the scene's motion.  Lists from the oracle's selector and tracker, max_error
    1.0, 256 hypotheses.  Printed, not asserted (this restatement, seed 0):
        320x240_w7:  tracked 145, inside the block 25 (25 flagged, 0 of them rejected by the forward-backward check), outside 107 (0 flagged)
        640x480_w15: tracked 292, inside the block 36 (36 flagged, 0 of them rejected by the forward-backward check), outside 236 (0 flagged)"""
    from oracle import klt_oracle as ko
    name, width, height, window, levels, ss, block, n = case
    f0, f1 = moving_block_pair(width, height, block)
    p = params_from_tc(make_tc(levels=levels, ss=ss, window=window))
    fin = ko.select_good_features(p, f0.astype(np.float32), n)
    track = oracle_tracker(ko, p, f0, f1)
    fwd = track(fin.copy(), 1, 2)
    out, model = motion_check_expected(fin, fwd, width, height, max_error=1.0, hypotheses=256)
    fb_out = fb_compose(track, fin, 1.0)[0]
    tracked = (fin["val"] >= 0) & (fwd["val"] == KLT_TRACKED)
    inside, outside = block_sides(fin, block, window)
    flagged = out["val"] == KLT_MODEL_OUTLIER
    fb_rejected = tracked & (fb_out["val"] != KLT_TRACKED)
    print("%s: tracked %d, inside the block %d (%d flagged, %d of them rejected by the forward-backward check), outside %d (%d flagged); "
          "model valid %d, %d of %d candidates inliers, hypothesis %d"
          % (name, tracked.sum(), (tracked & inside).sum(), (tracked & inside & flagged).sum(), (tracked & inside & fb_rejected).sum(),
             (tracked & outside).sum(), (tracked & outside & flagged).sum(), model["valid"], model["n_inliers"], model["n_candidates"],
             model["hypothesis"]))
    assert model["valid"] == 1
    assert (tracked & inside).sum() >= 10
    assert flagged[tracked & inside].all()
    assert not flagged[tracked & outside].any()
    assert (flagged & (fb_out["val"] == KLT_TRACKED)).any(), "every feature the model flags is rejected by the forward-backward check too"
    # the model is the background's motion
    A, t = model_affine(model)
    assert np.abs(A - np.eye(2)).max() < 5e-3 and abs(t[0] - 1.3) < 0.5 and abs(t[1] + 0.8) < 0.5
    assert np.array_equal(out[~flagged], fwd[~flagged])
    assert abs(BLOCK_MOTION[0] - 1.3) > 3 and abs(BLOCK_MOTION[1] + 0.8) > 3


KNOWN = [(n, size) for n in (3, 64, 65, 4097, 5000) for size in ((320, 240), (1920, 1080), (4096, 2160))]


@pytest.mark.parametrize("n,size", KNOWN, ids=["n%d_%dx%d" % (n, s[0], s[1]) for n, s in KNOWN])
def test_known_answer(n, size):
    """out = A in + t rounded to f32, the first quarter displaced by 5 px, max_error 0.5: exactly the displaced quarter is flagged and the
    returned map reproduces every inlier's `out` position to within 1e-3 px (four f32 half-ulps at 4096, the input's own rounding).
    Worst over these fifteen cases on this restatement: 1.4e-4 px (n = 64 at 4096x2160, where an f32 half-ulp is 2.4e-4)."""
    ncols, nrows = size
    fin, fout, A, t, moved = synthetic_lists(n, ncols, nrows, seed=1000 + n)
    kw = dict(max_error=0.5, min_inliers=3 if n == 3 else 8)
    out, model = motion_check_expected(fin, fout, ncols, nrows, **kw)
    assert model["valid"] == 1 and model["n_candidates"] == n
    flagged = out["val"] == KLT_MODEL_OUTLIER
    assert np.array_equal(flagged, moved)
    assert model["n_inliers"] == n - moved.sum()
    assert np.array_equal(out[~flagged], fout[~flagged])
    assert (out["x"][flagged] == -1).all() and (out["y"][flagged] == -1).all() and np.array_equal(out["aux"], fout["aux"])
    A2, t2 = model_affine(model)
    p = np.stack([fin["x"], fin["y"]]).astype(np.float64)[:, ~flagged]
    q = A2 @ p + t2[:, None]
    err = max(np.abs(q[0] - fout["x"][~flagged]).max(), np.abs(q[1] - fout["y"][~flagged]).max())
    print("n %d at %dx%d: worst |A p + t - out| over the inliers %.3g px" % (n, ncols, nrows, err))
    assert err <= 1e-3
    # the same seed gives the same bytes; another seed may pick another hypothesis but flags the same records
    out_b, model_b = motion_check_expected(fin, fout, ncols, nrows, **kw)
    assert out_b.tobytes() == out.tobytes() and model_b.tobytes() == model.tobytes()
    out_c, model_c = motion_check_expected(fin, fout, ncols, nrows, seed=12345, **kw)
    assert model_c["valid"] == 1 and np.array_equal(out_c["val"] == KLT_MODEL_OUTLIER, moved)


def _no_model(fin, fout, ncols, nrows, m, **kw):
    out, model = motion_check_expected(fin, fout, ncols, nrows, **kw)
    assert out.tobytes() == np.ascontiguousarray(fout, FEAT_DTYPE).tobytes()
    want = np.zeros((), MODEL_DTYPE)
    want["n_candidates"], want["hypothesis"] = m, -1
    want["pad"] = ncols | nrows << 16
    assert model.tobytes() == want.tobytes(), model
    return model


def test_no_model_leaves_out_alone():
    """valid = 0 with `out` byte-identical: too few candidates, all candidates collinear, one hypothesis with a repeated pick, and a
    best score below min_inliers"""
    ncols, nrows = 320, 240
    fin, fout, _, _, _ = synthetic_lists(64, ncols, nrows, seed=5)
    _no_model(fin[:7], fout[:7], ncols, nrows, 7)                                        # m < min_inliers
    x = np.arange(40, dtype=np.float64) * 5 + 20                                         # collinear: every area is 0
    _no_model(records(x, 0.5 * x + 10, 3), records(x + 1, 0.5 * x + 11), ncols, nrows, 40)
    seed = next(s for s in range(1000) if len(set(picks(s, 0, 64))) < 3)                 # hypothesis 0 picks one candidate twice
    _no_model(fin, fout, ncols, nrows, 64, hypotheses=1, seed=seed)
    rs = np.random.RandomState(9)                                                        # no common motion at all: the best score is tiny
    a = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1)
    b = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64))
    _no_model(a, b, ncols, nrows, 64, max_error=0.01, min_inliers=8)


def test_refit_that_fails_keeps_the_hypothesis():
    """valid = 2: min_area = 0 lets a degenerate hypothesis count; on collinear integer positions every number of it is an exact 0, every
    candidate is an inlier (0 <= 0), the normal equations are singular with an exact determinant 0, and the hypothesis is kept"""
    x = np.arange(20, dtype=np.float64) * 4 + 40
    fin, fout = records(x, x + 8, 1), records(x + 2, x + 10)
    out, model = motion_check_expected(fin, fout, 320, 240, min_area=0.0, hypotheses=5)
    assert model["valid"] == 2 and model["d"] == 0 and model["n_inliers"] == 20 and model["hypothesis"] == 0
    assert out.tobytes() == fout.tobytes() and model_affine(model) is None


def test_records_that_are_not_candidates_keep_their_bytes_and_are_never_sampled():
    """lost in `in`; each negative status in `out`; val > 0 (a slot a replacement refilled); NaN / +-inf / negative / >= ncols coordinates"""
    ncols, nrows = 320, 240
    fin, fout, _, _, moved = synthetic_lists(300, ncols, nrows, seed=8)
    idx = non_candidate_kinds(fin, fout, ncols, nrows, start=2, step=7)
    assert len(idx) == 11 + 24
    cand = candidate_mask(fin, fout, ncols, nrows)
    assert not cand[idx].any() and cand.sum() == 300 - len(idx)
    out, model = motion_check_expected(fin, fout, ncols, nrows, max_error=0.5)
    assert model["valid"] == 1 and model["n_candidates"] == cand.sum()
    assert out[idx].tobytes() == fout[idx].tobytes()                                     # (NaN bytes included)
    assert np.array_equal(out["val"][cand] == KLT_MODEL_OUTLIER, moved[cand])
    # never sampled: garbage coordinates in the non-candidates change nothing
    fin2, fout2 = fin.copy(), fout.copy()
    fin2["x"][idx], fout2["y"][idx] = 7e8, -3e9
    fin2["val"][idx] = np.where(cand[idx], fin2["val"][idx], -1)
    out2, model2 = motion_check_expected(fin2, fout2, ncols, nrows, max_error=0.5)
    assert model2.tobytes() == model.tobytes() and np.array_equal(out2["val"], out["val"])


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 5000])
def test_picks_stay_below_m(m):
    h = np.arange(65536, dtype=np.uint64)
    for seed in (0, 0xFFFFFFFF):
        for j in range(3):
            x = (np.uint64(3) * h + np.uint64(j)) & np.uint64(0xFFFFFFFF)
            for _ in range(2):                                           # mix(seed ^ mix(.)), vectorised
                x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
                x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
                x ^= x >> np.uint64(16)
                if _ == 0:
                    x ^= np.uint64(seed)
            r = (x * np.uint64(m)) >> np.uint64(32)
            assert r.max() < m
            assert int(r[5]) == picks(seed, 5, m)[j] and int(r[65535]) == picks(seed, 65535, m)[j]
    assert mulhi32(0xFFFFFFFF, m) == m - 1


def test_mix_is_the_finaliser_of_the_header():
    x = 0x12345678
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
    assert mix(0x12345678) == x and mix(0) == 0 and mix(0x112345678) == x          # uint32 arithmetic


def test_status_code_parameters_and_defaults():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState
    from pyfeaturetrack_amd.params import model_params_from_tc
    assert kltState.KLT_MODEL_OUTLIER == -7 == KLT_MODEL_OUTLIER
    tc = KLT_TrackingContext()
    assert tc.motionModelCheck is None and tc.model_max_error == 1.0 and tc.model_hypotheses == 256 and tc.model_seed == 0
    assert tc.model_min_inliers == 8
    m = model_params_from_tc(tc, 320, 240)
    assert (m.mode, m.ncols, m.nrows, m.hypotheses, m.seed, m.min_inliers, m.max_error, m.min_area) == (0, 320, 240, 256, 0, 8, 1.0, 1.0)
    tc.motionModelCheck = "affine"
    tc.model_max_error, tc.model_hypotheses, tc.model_seed, tc.model_min_inliers = 0.5, 1001, 77, 5
    m = model_params_from_tc(tc, 320, 240)
    assert (m.mode, m.ncols, m.nrows, m.hypotheses, m.seed, m.min_inliers, m.max_error, m.min_area) == (1, 320, 240, 1001, 77, 5, 0.5, 1.0)

    class Foreign:                       # a context made elsewhere has none of the fields
        affineConsistencyCheck = -1
    assert model_params_from_tc(Foreign(), 64, 48).mode == 0


def test_value_errors_before_any_device_work():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import model_params_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    img = np.zeros((64, 64), np.uint8)
    bad = [dict(motionModelCheck="homography"), dict(motionModelCheck=True), dict(motionModelCheck="affine", affineConsistencyCheck=2),
           dict(motionModelCheck="affine", model_hypotheses=0), dict(motionModelCheck="affine", model_hypotheses=65537),
           dict(motionModelCheck="affine", model_min_inliers=2), dict(motionModelCheck="affine", model_max_error=-1.0),
           dict(motionModelCheck="affine", model_max_error=float("nan")), dict(motionModelCheck="affine", model_seed=-1)]
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        for attrs in bad:
            tc = KLT_TrackingContext()
            for k, v in attrs.items():
                setattr(tc, k, v)
            with pytest.raises(ValueError, match="motionModelCheck|model_"):
                model_params_from_tc(tc)
            with pytest.raises(ValueError, match="motionModelCheck|model_"):
                KLTTrackFeatures(tc, img, img, [KLT_Feature() for _ in range(4)])
            with pytest.raises(ValueError, match="motionModelCheck|model_"):
                KLTTrackSequence(tc, [img, img], 4)
            assert "_klt_ctx" not in tc.__dict__                              # no device context was asked for
    finally:
        trk.KLT_verbose = verbose


def test_print_tracking_context_unchanged(capsys):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    KLTPrintTrackingContext(tc)
    plain = capsys.readouterr().out
    tc.motionModelCheck, tc.model_max_error = "affine", 0.25
    KLTPrintTrackingContext(tc)
    with_check = capsys.readouterr().out
    assert "motionModel" not in plain and "model_" not in plain
    assert plain.split("\n", 1)[1] == with_check.split("\n", 1)[1]          # (the first line is the object's repr)


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi, backend
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_set_model_params", "klt_motion_check_async", "klt_motion_check_batch_async", "klt_motion_check",
                 "klt_motion_model_affine", "klt_motion_check_path"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_abi.KltMotionModel) == 80 == 5 * ctypes.sizeof(_abi.KltFeat) and ctypes.sizeof(_abi.KltModelParams) == 32
    assert backend.MODEL_DTYPE == MODEL_DTYPE and backend.MODEL_DTYPE.itemsize == 80
    assert [f[0] for f in _abi.KltMotionModel._fields_] == list(MODEL_DTYPE.names)
    assert [getattr(_abi.KltMotionModel, k).offset for k in MODEL_DTYPE.names] == [MODEL_DTYPE.fields[k][1] for k in MODEL_DTYPE.names]
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11


def test_the_host_side_division_is_the_restatements():
    """klt_motion_model_affine (host only, no GPU): the uncentred map of a record, the same numbers as model_expected.model_affine"""
    from pyfeaturetrack_amd import backend
    fin, fout, A, t, moved = synthetic_lists(65, 1920, 1080, seed=3)
    _, model = motion_check_expected(fin, fout, 1920, 1080, max_error=0.5)
    A1, t1 = backend.model_affine(model)
    A2, t2 = model_affine(model)
    assert np.array_equal(A1, A2) and np.array_equal(t1, t2)
    assert np.abs(A1 - A).max() < 1e-6 and np.abs(t1 - t).max() < 1e-3
    assert backend.model_affine(np.zeros((), MODEL_DTYPE)) == (None, None)
    s = backend.model_summary(model)
    assert sorted(s) == ["A", "candidates", "hypothesis", "inliers", "t", "valid"] and s["valid"] == 1 and s["candidates"] == 65
