"""The homography check's rule (include/klt_gpu.h, "homography check") without a GPU: its numpy restatement
(tests/homography_expected.py) on the rotation and plane scenes, the translation, every way to end without a model and collinear
candidates; what the affine and the epipolar rule do on the same lists; the Python layer's parameters, refusals, printing and struct sizes.
tests/test_gpu_homography.py compares the device with the same restatement byte for byte."""
import ctypes

import numpy as np
import pytest

from epipolar_expected import epipolar_check_expected, parallax_lists, scale_of, translation_lists, working
from homography_expected import (DEFAULTS, HOMOGRAPHY_DTYPE, KLT_HOMOGRAPHY_OUTLIER, collinear_lists, homography_check_expected,
                                 homography_matrix, normal_matrix, null9, picks, rows_of, scene, transfer_error)
from model_expected import KLT_MODEL_OUTLIER, KLT_TRACKED, candidate_mask, motion_check_expected, non_candidate_kinds, records

SCENES = [(name, seed) for name in ("rotation", "plane") for seed in (11, 12)]
_CACHE = {}


def scene_result(name, seed):
    """the scene and the rule's answer on it at the defaults, computed once"""
    if (name, seed) not in _CACHE:
        fin, fout, moved, H = scene(name, seed)
        for a in (fin, fout, moved):
            a.setflags(write=False)
        _CACHE[name, seed] = (fin, fout, moved, H) + homography_check_expected(fin, fout, 1920, 1080)
    return _CACHE[name, seed]


# ---------------------------------------------------------------------------------------------------------------- the pieces
def test_null9_on_four_correspondences_returns_the_homography():
    H = np.array([[0.9, 0.05, 0.1], [-0.04, 1.1, -0.2], [0.2, -0.1, 1.0]])
    p = np.array([[-0.7, -0.5], [0.6, -0.4], [0.5, 0.7], [-0.6, 0.3]])
    q = (H @ np.c_[p, np.ones(4)].T).T
    q = q[:, :2] / q[:, 2:]
    A = rows_of(p[:, 0], p[:, 1], q[:, 0], q[:, 1])
    assert A.shape == (8, 9)
    assert np.array_equal(A[0], [p[0, 0], p[0, 1], 1, 0, 0, 0, -(q[0, 0] * p[0, 0]), -(q[0, 0] * p[0, 1]), -q[0, 0]])
    assert np.array_equal(A[1], [0, 0, 0, p[0, 0], p[0, 1], 1, -(q[0, 1] * p[0, 0]), -(q[0, 1] * p[0, 1]), -q[0, 1]])
    h = null9(A)
    assert h is not None and np.abs(A @ h).max() <= 1e-12 * np.abs(h).max()
    assert np.allclose(h / h[8], H.ravel(), rtol=0, atol=1e-12)
    # a repeated pick leaves two exactly zero rows: null9 fails, with no special case
    twice = rows_of(p[[0, 1, 2, 0], 0], p[[0, 1, 2, 0], 1], q[[0, 1, 2, 0], 0], q[[0, 1, 2, 0], 1])
    assert null9(twice) is None


def test_picks_are_four_per_hypothesis():
    from model_expected import mix, mulhi32
    assert picks(7, 3, 1000) == tuple(mulhi32(mix(7 ^ mix(12 + j)), 1000) for j in range(4))
    assert all(0 <= r < 5 for h in range(64) for r in picks(0, h, 5))


def test_the_normal_matrix_is_the_rows_least_squares():
    fin, fout, _, _ = scene("rotation", 11)
    px, py, qx, qy = working(fin, fout, np.ones(len(fin), bool), 1920, 1080)
    inl = np.ones(len(px), bool)
    inl[::7] = False
    M = normal_matrix(px, py, qx, qy, inl)
    rows = rows_of(px, py, qx, qy).reshape(len(px), 2, 9)[inl].reshape(-1, 9)
    assert np.allclose(M, rows.T @ rows, rtol=1e-12, atol=1e-12)
    assert np.array_equal(M, M.T)
    zeros = np.concatenate([M[0:3, 3:6].ravel(), M[3:6, 0:3].ravel()])
    assert not zeros.any() and not np.signbit(zeros).any()               # the structural zeros are +0.0


# ---------------------------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("name,seed", SCENES)
def test_every_static_track_is_kept_and_every_displaced_one_flagged(name, seed):
    """noise of 0.1 px against a threshold of 1 px, displacements of at least 3 px per axis: nothing is near the threshold"""
    fin, fout, moved, H, out, rec = scene_result(name, seed)
    flag = out["val"] == KLT_HOMOGRAPHY_OUTLIER
    print("%s %d: valid %d, %d static (%d kept), %d moved (%d flagged), hypothesis %d with %d inliers" % (
        name, seed, rec["valid"], (~moved).sum(), (~flag & ~moved).sum(), moved.sum(), (flag & moved).sum(), rec["hypothesis"],
        rec["hypothesis_inliers"]))
    assert rec["valid"] == 1 and rec["n_candidates"] == len(fin)
    assert not (flag & ~moved).any(), "static tracks flagged"
    assert (flag | ~moved).all(), "displaced tracks kept"
    assert rec["n_inliers"] == (~moved).sum()
    assert np.array_equal(out["aux"], fout["aux"]) and (out["x"][flag] == -1).all() and (out["y"][flag] == -1).all()
    assert out[~flag].tobytes() == fout[~flag].tobytes()


@pytest.mark.parametrize("name,seed", SCENES)
def test_the_pixel_matrix_transfers_every_kept_track_within_the_threshold(name, seed):
    fin, fout, moved, H, out, rec = scene_result(name, seed)
    Hm = homography_matrix(rec).reshape(3, 3)
    assert abs(np.sum(Hm * Hm) - 1.0) <= 1e-14
    c = Hm @ np.array([960.0, 540.0, 1.0])
    assert c[2] > 0                                                      # the third coordinate is positive at the image centre
    kept = out["val"] == KLT_TRACKED
    err = transfer_error(Hm, fin, fout)
    print("%s %d: largest transfer error of a kept track %.3f px, smallest of a flagged one %.3f px" % (name, seed, err[kept].max(), err[~kept].min()))
    assert err[kept].max() <= 1.0 and err[~kept].min() > 1.0
    # the scene's own homography explains every static track up to the noise: a Rayleigh variable of 0.1 px exceeds 0.6 px with
    # probability exp(-18)
    assert transfer_error(H, fin, fout)[~moved].max() <= 0.6


@pytest.mark.parametrize("name,seed", SCENES)
def test_the_other_two_rules_fail_on_the_same_lists(name, seed):
    """what the check is for: the affine rule flags static tracks, the epipolar rule keeps displaced ones (counts: DESIGN.md section 9i)"""
    fin, fout, moved, H, out, rec = scene_result(name, seed)
    aff, _ = motion_check_expected(fin, fout, 1920, 1080)
    epi, _ = epipolar_check_expected(fin, fout, 1920, 1080)
    static_flagged = int(((aff["val"] == KLT_MODEL_OUTLIER) & ~moved).sum())
    moved_kept = int(((epi["val"] == KLT_TRACKED) & moved).sum())
    print("%s %d: the affine rule flags %d of %d static tracks, the epipolar rule keeps %d of %d displaced ones" % (
        name, seed, static_flagged, (~moved).sum(), moved_kept, moved.sum()))
    assert static_flagged > 0
    assert moved_kept > 0


def test_a_translation_is_found_exactly():
    fin, fout = translation_lists(64, 320, 240, 5)
    out, rec = homography_check_expected(fin, fout, 320, 240)
    assert rec["valid"] == 1 and rec["n_inliers"] == 64 and out.tobytes() == fout.tobytes()
    s = scale_of(320, 240)
    h = rec["h"]
    # identity plus (3 s, -2 s): the zeros and the diagonal exactly, the translation to the rounding of the refit's sums and of the
    # division here (it came out one unit in the last place off)
    assert h[0] == h[4] == h[8] > 0 and not h[[1, 3, 6, 7]].any()
    assert abs(h[2] / h[8] - 3 * s) <= 2 * np.spacing(3 * s) and abs(h[5] / h[8] + 2 * s) <= 2 * np.spacing(2 * s)
    Hm = homography_matrix(rec).reshape(3, 3)
    assert np.allclose(Hm / Hm[2, 2], [[1, 0, 3], [0, 1, -2], [0, 0, 1]], rtol=0, atol=1e-12)


def test_every_way_to_end_without_a_model():
    fin, fout, _, _ = scene("rotation", 11)
    # fewer candidates than min_inliers
    out, rec = homography_check_expected(fin[:7], fout[:7], 1920, 1080)
    assert rec["valid"] == 0 and rec["n_candidates"] == 7 and rec["hypothesis"] == -1 and out.tobytes() == fout[:7].tobytes()
    assert not rec["h"].any() and rec["n_inliers"] == 0 and rec["hypothesis_inliers"] == 0
    assert int(np.array(rec["pad"]).view(np.uint32)) == 1920 | 1080 << 16
    # no hypothesis gathers min_inliers: unrelated positions under a threshold of 0.01 px
    rs = np.random.RandomState(9)
    rin = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1)
    rout = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64))
    out, rec = homography_check_expected(rin, rout, 320, 240, max_error=0.01, hypotheses=64)
    assert rec["valid"] == 0 and rec["n_candidates"] == 64 and rec["hypothesis"] == -1 and out.tobytes() == rout.tobytes()
    # ... and the noisy scene itself under that threshold
    out, rec = homography_check_expected(fin[60:124], fout[60:124], 1920, 1080, max_error=0.01, hypotheses=64)
    assert rec["valid"] == 0 and out.tobytes() == fout[60:124].tobytes()
    # an empty list
    out, rec = homography_check_expected(fin[:0], fout[:0], 1920, 1080)
    assert rec["valid"] == 0 and rec["n_candidates"] == 0 and len(out) == 0


def test_collinear_candidates_flag_nothing():
    """a family of homographies fits collinear correspondences: whichever member is found, it fits them all; on exact integer positions
    every 8x9 matrix is exactly singular instead and there is no model.  (With noise on frame 2 a line of candidates is a limit of the
    check, not a safe case: DESIGN.md section 9i has the figures.)"""
    for seed in (3, 4):
        fin, fout = collinear_lists(40, 1920, 1080, seed)
        out, rec = homography_check_expected(fin, fout, 1920, 1080)
        print("collinear %d: valid %d, %d of %d inliers" % (seed, rec["valid"], rec["n_inliers"], rec["n_candidates"]))
        assert out.tobytes() == fout.tobytes()
        assert rec["valid"] == 1 and rec["n_inliers"] == 40
    k = np.arange(40)
    fin, fout = records(16 + 7 * k, 30 + 3 * k), records(19 + 7 * k, 28 + 3 * k)
    out, rec = homography_check_expected(fin, fout, 320, 240)
    assert out.tobytes() == fout.tobytes() and rec["valid"] == 0 and rec["n_candidates"] == 40


def test_a_scene_with_parallax_is_no_homography():
    """the limit the README names: most static tracks of a camera that translates through depth are flagged"""
    fin, fout, moved = parallax_lists("oblique", 11)
    out, rec = homography_check_expected(fin, fout, 1920, 1080)
    flagged = int(((out["val"] == KLT_HOMOGRAPHY_OUTLIER) & ~moved).sum())
    print("oblique parallax: %d of %d static tracks flagged" % (flagged, (~moved).sum()))
    assert flagged > 0.5 * (~moved).sum()


# ---------------------------------------------------------------------------------------------------------------- fixed behaviours
def test_the_same_seed_gives_the_same_bytes_and_the_seed_matters():
    fin, fout, _, _ = scene("plane", 12)
    a = homography_check_expected(fin, fout, 1920, 1080, hypotheses=64, seed=5)
    b = homography_check_expected(fin.copy(), fout.copy(), 1920, 1080, hypotheses=64, seed=5)
    c = homography_check_expected(fin, fout, 1920, 1080, hypotheses=64, seed=6)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[1]["hypothesis"] != c[1]["hypothesis"] or a[1].tobytes() != c[1].tobytes()


def test_every_kind_of_non_candidate_leaves_the_result_unchanged():
    fin, fout, _, _ = scene("rotation", 12)
    fin, fout = fin[:200], fout[:200]
    want_out, want_rec = homography_check_expected(fin, fout, 1920, 1080, hypotheses=64)
    assert want_rec["valid"] == 1 and (want_out["val"] == KLT_HOMOGRAPHY_OUTLIER).any()
    extra = 50
    ein, eout = fin[:extra].copy(), fout[:extra].copy()
    kinds = non_candidate_kinds(ein, eout, 1920, 1080)
    assert 30 <= len(kinds) < extra
    eout["val"][len(kinds):] = KLT_HOMOGRAPHY_OUTLIER             # ... and this check's own status in the remaining ones
    at = np.arange(extra) * 4
    big_in, big_out = np.insert(fin, at, ein), np.insert(fout, at, eout)
    slots = at + np.arange(extra)
    assert big_out[slots].tobytes() == eout.tobytes() and not candidate_mask(big_in, big_out, 1920, 1080)[slots].any()
    out, rec = homography_check_expected(big_in, big_out, 1920, 1080, hypotheses=64)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[slots].tobytes() == eout.tobytes()
    assert np.delete(out, slots).tobytes() == want_out.tobytes()


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_status_code_parameters_and_defaults():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState
    from pyfeaturetrack_amd.params import homography_params_from_tc
    assert kltState.KLT_HOMOGRAPHY_OUTLIER == -9 == KLT_HOMOGRAPHY_OUTLIER
    tc = KLT_TrackingContext()
    assert tc.homographyCheck is False
    assert (tc.homography_max_error, tc.homography_hypotheses, tc.homography_seed, tc.homography_min_inliers) == (1.0, 256, 0, 8)
    assert DEFAULTS == dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0)
    e = homography_params_from_tc(tc, 320, 240)
    assert (e.mode, e.ncols, e.nrows, e.hypotheses, e.seed, e.min_inliers, e.max_error) == (0, 320, 240, 256, 0, 8, 1.0)
    tc.homographyCheck = True
    tc.homography_max_error, tc.homography_hypotheses, tc.homography_seed, tc.homography_min_inliers = 0.5, 1001, 77, 4
    e = homography_params_from_tc(tc, 320, 240)
    assert (e.mode, e.ncols, e.nrows, e.hypotheses, e.seed, e.min_inliers, e.max_error) == (1, 320, 240, 1001, 77, 4, 0.5)

    class Foreign:                       # a context made elsewhere has none of the fields
        affineConsistencyCheck = -1
    assert homography_params_from_tc(Foreign(), 64, 48).mode == 0
    f = Foreign()
    f.homographyCheck = True             # ... and the defaults are read with getattr
    e = homography_params_from_tc(f, 64, 48)
    assert (e.mode, e.hypotheses, e.seed, e.min_inliers, e.max_error) == (1, 256, 0, 8, 1.0)


def test_value_errors_before_any_device_work():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import homography_params_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    img = np.zeros((64, 64), np.uint8)
    on = dict(homographyCheck=True)
    bad = [dict(homographyCheck="on"), dict(homographyCheck=1), dict(on, motionModelCheck="affine"), dict(on, epipolarCheck=True),
           dict(on, affineConsistencyCheck=0), dict(on, affineConsistencyCheck=2), dict(on, homography_hypotheses=0),
           dict(on, homography_hypotheses=65537), dict(on, homography_min_inliers=3), dict(on, homography_max_error=-1.0),
           dict(on, homography_max_error=float("nan")), dict(on, homography_seed=-1), dict(on, homography_seed=2 ** 32)]
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        for attrs in bad:
            tc = KLT_TrackingContext()
            for k, v in attrs.items():
                setattr(tc, k, v)
            with pytest.raises(ValueError, match="homography"):
                homography_params_from_tc(tc)
            with pytest.raises(ValueError, match="homography|affineConsistencyCheck"):
                KLTTrackFeatures(tc, img, img, [KLT_Feature() for _ in range(4)])
            with pytest.raises(ValueError, match="homography|affineConsistencyCheck"):
                KLTTrackSequence(tc, [img, img], 4)
            assert "_klt_ctx" not in tc.__dict__                              # no device context was asked for
        tc = KLT_TrackingContext()
        tc.homographyCheck = True
        with pytest.raises(ValueError, match="homography check takes frames"):
            homography_params_from_tc(tc, 65536, 100)
        for switches in (dict(motionModelCheck="homography"), dict(on, motionModelCheck="homography")):      # still a refusal
            tc = KLT_TrackingContext()
            for k, v in switches.items():
                setattr(tc, k, v)
            with pytest.raises(ValueError, match="motionModelCheck"):
                KLTTrackFeatures(tc, img, img, [KLT_Feature() for _ in range(4)])
            assert "_klt_ctx" not in tc.__dict__
    finally:
        trk.KLT_verbose = verbose


def test_print_tracking_context_names_the_check_only_when_it_is_on(capsys):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    KLTPrintTrackingContext(tc)
    plain = capsys.readouterr().out
    assert "homography" not in plain
    tc.homography_max_error = 0.25                           # (a parameter alone prints nothing)
    KLTPrintTrackingContext(tc)
    assert capsys.readouterr().out.split("\n", 1)[1] == plain.split("\n", 1)[1]
    tc.homographyCheck = True
    KLTPrintTrackingContext(tc)
    on = capsys.readouterr().out
    for line in ("\thomographyCheck = True", "\thomography_max_error = 0.25", "\thomography_hypotheses = 256", "\thomography_seed = 0",
                 "\thomography_min_inliers = 8"):
        assert line in on
    assert "epipolar" not in on


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi, backend
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_set_homography_params", "klt_homography_check_async", "klt_homography_check_batch_async", "klt_homography_check",
                 "klt_homography_matrix", "klt_homography_check_path"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_abi.KltHomographyModel) == 96 == 6 * ctypes.sizeof(_abi.KltFeat) and ctypes.sizeof(_abi.KltHomographyParams) == 28
    assert backend.HOMOGRAPHY_DTYPE == HOMOGRAPHY_DTYPE and backend.HOMOGRAPHY_DTYPE.itemsize == 96
    assert [f[0] for f in _abi.KltHomographyModel._fields_] == list(HOMOGRAPHY_DTYPE.names)
    assert [getattr(_abi.KltHomographyModel, k).offset for k in HOMOGRAPHY_DTYPE.names] == [HOMOGRAPHY_DTYPE.fields[k][1] for k in HOMOGRAPHY_DTYPE.names]
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11                       # additive: the version stays


def test_the_host_matrix_equals_its_restatement_and_refuses_what_it_must():
    from pyfeaturetrack_amd import _abi, backend
    lib = _abi.load_library()
    H = (ctypes.c_double * 9)()
    rec = _abi.KltHomographyModel()
    assert lib.klt_homography_matrix(None, H) == -1 and lib.klt_homography_matrix(ctypes.byref(rec), None) == -1
    assert lib.klt_homography_matrix(ctypes.byref(rec), H) == -3             # valid == 0
    rec.valid, rec.pad = 1, 320 | 240 << 16
    assert lib.klt_homography_matrix(ctypes.byref(rec), H) == -3             # h all zero: no norm
    rec.h[0] = float("inf")
    assert lib.klt_homography_matrix(ctypes.byref(rec), H) == -3             # not finite
    for name, seed in SCENES:
        want = scene_result(name, seed)[5]
        assert np.array_equal(backend.homography_matrix(want), homography_matrix(want).reshape(3, 3))
    neg = scene_result("rotation", 11)[5].copy()
    neg["h"] = -neg["h"]                                                     # the sign of h does not matter
    assert np.array_equal(backend.homography_matrix(neg), homography_matrix(scene_result("rotation", 11)[5]).reshape(3, 3))
    assert backend.homography_matrix(np.zeros((), HOMOGRAPHY_DTYPE)) is None
