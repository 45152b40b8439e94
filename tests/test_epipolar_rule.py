"""The epipolar check's rule (include/klt_gpu.h, "epipolar check") on the CPU: the numpy restatement
(tests/epipolar_expected.py) against linear algebra it does not use, against the parallax scene it was made for, and on every way it has
of finding no model; the Python parameters, the host-side entry point and the exports.  No test here needs a GPU."""
import ctypes

import numpy as np
import pytest

from epipolar_expected import (DEFAULTS, EPIPOLAR_DTYPE, KLT_EPIPOLAR_OUTLIER, SCENES, candidate_mask, epipolar_check_expected,
                               epipolar_matrix, free_index, hypothesis_of, inliers, null9, parallax_lists, picks, refit, rows_of,
                               scale_of, scores_expected, threshold2, translation_lists, working)
from model_expected import FEAT_DTYPE, KLT_MODEL_OUTLIER, KLT_TRACKED, mix, motion_check_expected, mulhi32, non_candidate_kinds, records

SCENE_SEEDS = (11, 12)


# ---------------------------------------------------------------------------------------------------------------- null9
def _unit(v):
    return v / np.linalg.norm(v)


def test_null9_is_the_null_vector_of_a_full_rank_matrix():
    rs = np.random.RandomState(1)
    for trial in range(20):
        A = rs.normal(size=(8, 9)) * 10.0 ** rs.randint(-3, 4)
        x = null9(A)
        assert x is not None and abs(x).max() < 9.0 ** 8
        v = np.linalg.svd(A)[2][-1]
        # cond(A) of a Gaussian 8x9 matrix stays below 1e3 here: residual and direction agree to that many ulps
        assert np.abs(A @ _unit(x)).max() <= 1e-12 * np.abs(A).max(), trial
        assert abs(abs(_unit(x) @ v) - 1.0) <= 1e-12, trial


def test_null9_fails_on_two_equal_rows_and_on_a_zero_or_infinite_entry():
    rs = np.random.RandomState(2)
    A = rs.normal(size=(8, 9))
    assert null9(A) is not None
    B = A.copy()
    B[6] = B[2]
    assert null9(B) is None                                  # an exactly zero row after the elimination
    B = A.copy()
    B[3] = 0.0
    assert null9(B) is None
    B = A.copy()
    B[1, 4] = np.inf
    assert null9(B) is None
    assert null9(np.full((8, 9), 5e-324)) is None            # subnormal pivots


def test_null9_does_not_depend_on_the_order_of_the_rows_beyond_rounding():
    rs = np.random.RandomState(3)
    A = rs.normal(size=(8, 9))
    x = _unit(null9(A))
    for trial in range(5):
        y = _unit(null9(A[rs.permutation(8)]))
        assert min(np.abs(x - y).max(), np.abs(x + y).max()) <= 1e-12


def test_null9_pivot_ties_go_to_the_smallest_row_then_column():
    """a matrix of +-1 entries: every pivot search of step 0 is a tie; the bits of |v| are compared, so the sign plays no part"""
    A = np.ones((8, 9))
    A[np.arange(8), np.arange(8)] = -1.0                    # rows differ: full rank
    x = null9(A)
    assert x is not None and np.abs(A @ x).max() == 0.0      # (small integers: exact)


def test_picks_take_eight_candidates_with_the_existing_hash():
    for seed, h, m in ((0, 0, 100), (7, 511, 8), (0xFFFFFFFF, 65535, 5000)):
        assert picks(seed, h, m) == tuple(mulhi32(mix(seed ^ mix(8 * h + j)), m) for j in range(8))
        assert all(0 <= r < m for r in picks(seed, h, m))


def test_the_working_scale():
    assert [scale_of(*s) for s in ((1, 1), (2, 2), (3, 2), (320, 240), (1920, 1080), (2048, 100), (2049, 100), (65535, 1))] == \
        [1.0, 1.0, 0.5, 2.0 ** -8, 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -15]
    fin, fout, _ = parallax_lists("oblique", 11)
    px, py, qx, qy = working(fin, fout, np.ones(len(fin), bool), 1920, 1080)
    assert max(abs(px).max(), abs(py).max(), abs(qx).max(), abs(qy).max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the parallax scene
@pytest.fixture(scope="module")
def scenes():
    """every scene and seed once: (in, out, moved, out after the check, record)"""
    got = {}
    for name in SCENES:
        for seed in SCENE_SEEDS:
            fin, fout, moved = parallax_lists(name, seed)
            out, rec = epipolar_check_expected(fin, fout, 1920, 1080)
            got[name, seed] = (fin, fout, moved, out, rec)
    return got


@pytest.mark.parametrize("seed", SCENE_SEEDS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_parallax_scene_keeps_the_static_tracks_and_flags_the_moved_ones(scenes, name, seed):
    fin, fout, moved, out, rec = scenes[name, seed]
    flag = out["val"] == KLT_EPIPOLAR_OUTLIER
    static = ~moved
    print("%s seed %d: %d tracks, static kept %d of %d, moved flagged %d of %d, valid %d, hypothesis %d with %d inliers, %d after the refit"
          % (name, seed, len(fin), (static & ~flag).sum(), static.sum(), (moved & flag).sum(), moved.sum(), rec["valid"], rec["hypothesis"],
             rec["hypothesis_inliers"], rec["n_inliers"]))
    assert rec["valid"] == 1 and rec["n_candidates"] == len(fin)
    assert (static & ~flag).sum() >= 0.98 * static.sum()
    assert (moved & flag).sum() >= 0.70 * moved.sum()
    assert rec["n_inliers"] == (~flag).sum()
    kept = ~flag
    assert out[kept].tobytes() == fout[kept].tobytes()
    assert (out["x"][flag] == -1).all() and (out["y"][flag] == -1).all() and np.array_equal(out["aux"], fout["aux"])


@pytest.mark.parametrize("seed", SCENE_SEEDS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_affine_check_rejects_the_static_tracks_of_the_parallax_scene(scenes, name, seed):
    """what the epipolar check is for: the planar rule finds a model and flags more than half of the tracks that did not move"""
    fin, fout, moved, _, _ = scenes[name, seed]
    out, model = motion_check_expected(fin, fout, 1920, 1080)
    flag = out["val"] == KLT_MODEL_OUTLIER
    print("%s seed %d: the affine rule flags %d of %d static tracks (valid %d)" % (name, seed, (flag & ~moved).sum(), (~moved).sum(), model["valid"]))
    assert model["valid"] == 1 and (flag & ~moved).sum() > 0.5 * (~moved).sum()


def test_the_matrix_in_pixels_annihilates_the_static_tracks(scenes):
    """klt_epipolar_matrix (host only, no GPU) against the restatement, and q^T F p ~ 0 in uncentred pixels"""
    from pyfeaturetrack_amd import backend
    for (name, seed), (fin, fout, moved, out, rec) in scenes.items():
        F = backend.epipolar_matrix(rec)
        want = epipolar_matrix(rec).reshape(3, 3)
        assert F.shape == (3, 3) and np.array_equal(F, want), (name, seed, F, want)
        assert abs(np.linalg.norm(F) - 1.0) <= 1e-15
        p = np.stack([fin["x"], fin["y"], np.ones(len(fin))]).astype(np.float64)
        q = np.stack([fout["x"], fout["y"], np.ones(len(fin))]).astype(np.float64)
        # Sampson distance in pixels of the tracks the check kept: the threshold of 1 px holds in these coordinates too
        a, b = F @ p, F.T @ q
        d = np.abs(np.einsum("in,in->n", q, a)) / np.sqrt(a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2)
        kept = out["val"] == KLT_TRACKED
        assert d[kept].max() <= 1.0 + 1e-9 and d[~kept].min() >= 1.0 - 1e-9, (name, seed, d[kept].max(), d[~kept].min())
    assert backend.epipolar_matrix(np.zeros((), EPIPOLAR_DTYPE)) is None and epipolar_matrix(np.zeros((), EPIPOLAR_DTYPE)) is None


# ---------------------------------------------------------------------------------------------------------------- no model
def _no_model(fin, fout, ncols, nrows, m, **kw):
    out, rec = epipolar_check_expected(fin, fout, ncols, nrows, **kw)
    want = np.zeros((), EPIPOLAR_DTYPE)
    want["hypothesis"], want["n_candidates"] = -1, m
    want["pad"] = ncols | nrows << 16
    assert rec.tobytes() == want.tobytes(), rec
    assert out.tobytes() == np.ascontiguousarray(fout, FEAT_DTYPE).tobytes()


def test_no_model_leaves_out_untouched():
    fin, fout, _ = parallax_lists("oblique", 11)
    _no_model(fin[:15], fout[:15], 1920, 1080, 15)                                               # m < min_inliers
    _no_model(fin[:7], fout[:7], 1920, 1080, 7, min_inliers=8)
    tin, tout = translation_lists(64, 320, 240, 3)                                               # every hypothesis degenerate
    cand = candidate_mask(tin, tout, 320, 240)
    px, py, qx, qy = working(tin, tout, cand, 320, 240)
    assert np.linalg.matrix_rank(rows_of(px, py, qx, qy)) <= 6
    assert (scores_expected(px, py, qx, qy, 64, 0, threshold2(1.0, 320, 240)) == -1).all()
    _no_model(tin, tout, 320, 240, 64)
    rs = np.random.RandomState(5)                                                                # best score below min_inliers
    rin = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64), 1)
    rout = records(rs.uniform(10, 300, 64), rs.uniform(10, 220, 64))
    cand = candidate_mask(rin, rout, 320, 240)
    px, py, qx, qy = working(rin, rout, cand, 320, 240)
    best = scores_expected(px, py, qx, qy, 64, 0, threshold2(0.01, 320, 240)).max()
    assert 8 <= best < 16                                    # (a hypothesis is an inlier of its own eight picks)
    _no_model(rin, rout, 320, 240, 64, hypotheses=64, max_error=0.01)


def test_degenerate_geometry_flags_less_never_a_kept_hypothesis():
    """valid == 2 needs a hypothesis that passes null9 while the normal equations of its inliers lose rank EXACTLY.  Attempts: a planar
    scene, a pure rotation, exactly eight candidates, eight candidates repeated.  Rounding in the 45 sums keeps every pivot of the refit
    away from zero: each gives valid 0 or 1.  (Exact integer positions do reach valid 2: check_draws_expected.valid2_lists, DESIGN.md
    section 9h.)"""
    rs = np.random.RandomState(8)
    n = 200
    x, y = rs.uniform(100, 1800, n), rs.uniform(100, 1000, n)
    seen = set()
    H = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])                  # a planar scene: a homography
    w = H @ np.stack([x, y, np.ones(n)])
    ang = 0.01                                                                                   # a pure rotation about y, focal length 1000
    xr = 1000 * ((x - 960) / 1000 + ang) / (1 - ang * (x - 960) / 1000) + 960
    yr = 1000 * ((y - 540) / 1000) / (1 - ang * (x - 960) / 1000) + 540
    e8 = records(x[:8], y[:8], 0, 0), records(x[:8] + 0.01 * (y[:8] - 500), y[:8] + 0.3, KLT_TRACKED, 0)
    cases = [("plane", records(x, y, 0, 0), records(w[0] / w[2], w[1] / w[2], KLT_TRACKED, 0), {}),
             ("rotation", records(x, y, 0, 0), records(xr, yr, KLT_TRACKED, 0), {}),
             ("eight", e8[0], e8[1], dict(min_inliers=8, hypotheses=4096)),
             ("eight twice", np.concatenate([e8[0], e8[0]]), np.concatenate([e8[1], e8[1]]), dict(min_inliers=8, hypotheses=512))]
    for name, fin, fout, kw in cases:
        out, rec = epipolar_check_expected(fin, fout, 1920, 1080, **kw)
        flagged = int((out["val"] == KLT_EPIPOLAR_OUTLIER).sum())
        print("%s: valid %d, %d of %d flagged" % (name, rec["valid"], flagged, len(fin)))
        seen.add(int(rec["valid"]))
        assert rec["valid"] in (0, 1)
        assert flagged <= 0.02 * len(fin)                    # every track follows ONE rigid motion: whatever F is found, it fits them
    assert 1 in seen


def test_the_free_index_and_the_refit():
    assert free_index(np.array([1.0, -3.0, 3.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0])) == 1       # ties to the smallest index, by magnitude
    fin, fout, moved = parallax_lists("oblique", 11)
    px, py, qx, qy = working(fin, fout, np.ones(len(fin), bool), 1920, 1080)
    t2 = threshold2(1.0, 1920, 1080)
    h = int(np.argmax(scores_expected(px, py, qx, qy, 64, 0, t2)))
    f = hypothesis_of(px, py, qx, qy, 0, h)
    inl = inliers(f, px, py, qx, qy, t2)
    g = refit(px, py, qx, qy, inl, f)
    # least squares with f_g free: no worse than the hypothesis on its own inliers, measured in the algebraic residual at f_g = 1
    rows = rows_of(px, py, qx, qy)[inl]
    k = free_index(f)
    assert np.sum((rows @ (g / g[k])) ** 2) <= np.sum((rows @ (f / f[k])) ** 2)


# ---------------------------------------------------------------------------------------------------------------- fixed behaviours
def test_the_same_seed_gives_the_same_bytes_and_the_seed_matters():
    fin, fout, _ = parallax_lists("forward", 12)
    a = epipolar_check_expected(fin, fout, 1920, 1080, hypotheses=64, seed=5)
    b = epipolar_check_expected(fin.copy(), fout.copy(), 1920, 1080, hypotheses=64, seed=5)
    c = epipolar_check_expected(fin, fout, 1920, 1080, hypotheses=64, seed=6)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[1]["hypothesis"] != c[1]["hypothesis"] or a[1].tobytes() != c[1].tobytes()


def test_every_kind_of_non_candidate_leaves_the_result_unchanged():
    fin, fout, _ = parallax_lists("oblique", 12)
    fin, fout = fin[:200], fout[:200]
    want_out, want_rec = epipolar_check_expected(fin, fout, 1920, 1080, hypotheses=64)
    assert want_rec["valid"] == 1 and (want_out["val"] == KLT_EPIPOLAR_OUTLIER).any()
    # the same lists with a record of every non-candidate kind put in front of every fourth record
    extra = 50
    ein, eout = fin[:extra].copy(), fout[:extra].copy()
    kinds = non_candidate_kinds(ein, eout, 1920, 1080)
    assert 30 <= len(kinds) < extra
    eout["val"][len(kinds):] = KLT_EPIPOLAR_OUTLIER               # ... and this check's own status in the remaining ones
    at = np.arange(extra) * 4
    big_in, big_out = np.insert(fin, at, ein), np.insert(fout, at, eout)
    slots = at + np.arange(extra)
    assert big_out[slots].tobytes() == eout.tobytes() and not candidate_mask(big_in, big_out, 1920, 1080)[slots].any()
    out, rec = epipolar_check_expected(big_in, big_out, 1920, 1080, hypotheses=64)
    assert rec.tobytes() == want_rec.tobytes()
    assert out[slots].tobytes() == eout.tobytes()
    assert np.delete(out, slots).tobytes() == want_out.tobytes()


def test_status_code_parameters_and_defaults():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState
    from pyfeaturetrack_amd.params import epipolar_params_from_tc
    assert kltState.KLT_EPIPOLAR_OUTLIER == -8 == KLT_EPIPOLAR_OUTLIER
    tc = KLT_TrackingContext()
    assert tc.epipolarCheck is False
    assert (tc.epipolar_max_error, tc.epipolar_hypotheses, tc.epipolar_seed, tc.epipolar_min_inliers) == (1.0, 512, 0, 16)
    assert DEFAULTS == dict(hypotheses=512, seed=0, min_inliers=16, max_error=1.0)
    e = epipolar_params_from_tc(tc, 320, 240)
    assert (e.mode, e.ncols, e.nrows, e.hypotheses, e.seed, e.min_inliers, e.max_error) == (0, 320, 240, 512, 0, 16, 1.0)
    tc.epipolarCheck = True
    tc.epipolar_max_error, tc.epipolar_hypotheses, tc.epipolar_seed, tc.epipolar_min_inliers = 0.5, 1001, 77, 9
    e = epipolar_params_from_tc(tc, 320, 240)
    assert (e.mode, e.ncols, e.nrows, e.hypotheses, e.seed, e.min_inliers, e.max_error) == (1, 320, 240, 1001, 77, 9, 0.5)

    class Foreign:                       # a context made elsewhere has none of the fields
        affineConsistencyCheck = -1
    assert epipolar_params_from_tc(Foreign(), 64, 48).mode == 0


def test_value_errors_before_any_device_work():
    from pyfeaturetrack_amd.klt import KLT_Feature, KLT_TrackingContext
    from pyfeaturetrack_amd.params import epipolar_params_from_tc
    from pyfeaturetrack_amd.trackFeatures import KLTTrackFeatures
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    from pyfeaturetrack_amd import trackFeatures as trk
    img = np.zeros((64, 64), np.uint8)
    on = dict(epipolarCheck=True)
    bad = [dict(epipolarCheck="on"), dict(epipolarCheck=1), dict(on, motionModelCheck="affine"), dict(on, affineConsistencyCheck=0),
           dict(on, affineConsistencyCheck=2), dict(on, epipolar_hypotheses=0), dict(on, epipolar_hypotheses=65537),
           dict(on, epipolar_min_inliers=7), dict(on, epipolar_max_error=-1.0), dict(on, epipolar_max_error=float("nan")),
           dict(on, epipolar_seed=-1), dict(on, epipolar_seed=2 ** 32)]
    verbose, trk.KLT_verbose = trk.KLT_verbose, 0
    try:
        for attrs in bad:
            tc = KLT_TrackingContext()
            for k, v in attrs.items():
                setattr(tc, k, v)
            with pytest.raises(ValueError, match="epipolar"):
                epipolar_params_from_tc(tc)
            with pytest.raises(ValueError, match="epipolar|affineConsistencyCheck"):
                KLTTrackFeatures(tc, img, img, [KLT_Feature() for _ in range(4)])
            with pytest.raises(ValueError, match="epipolar|affineConsistencyCheck"):
                KLTTrackSequence(tc, [img, img], 4)
            assert "_klt_ctx" not in tc.__dict__                              # no device context was asked for
        tc = KLT_TrackingContext()
        tc.epipolarCheck = True
        with pytest.raises(ValueError, match="epipolar check takes frames"):
            epipolar_params_from_tc(tc, 65536, 100)
    finally:
        trk.KLT_verbose = verbose


def test_print_tracking_context_names_the_check_only_when_it_is_on(capsys):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTPrintTrackingContext
    tc = KLT_TrackingContext()
    KLTPrintTrackingContext(tc)
    plain = capsys.readouterr().out
    assert "epipolar" not in plain
    tc.epipolar_max_error = 0.25                             # (a parameter alone prints nothing)
    KLTPrintTrackingContext(tc)
    assert capsys.readouterr().out.split("\n", 1)[1] == plain.split("\n", 1)[1]
    tc.epipolarCheck = True
    KLTPrintTrackingContext(tc)
    on = capsys.readouterr().out
    for line in ("\tepipolarCheck = True", "\tepipolar_max_error = 0.25", "\tepipolar_hypotheses = 512", "\tepipolar_seed = 0",
                 "\tepipolar_min_inliers = 16"):
        assert line in on


def test_abi_declares_the_entry_points():
    from pyfeaturetrack_amd import _abi, backend
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("klt_set_epipolar_params", "klt_epipolar_check_async", "klt_epipolar_check_batch_async", "klt_epipolar_check",
                 "klt_epipolar_matrix", "klt_epipolar_check_path"):
        assert name in _abi.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(_abi.KltEpipolarModel) == 96 == 6 * ctypes.sizeof(_abi.KltFeat) and ctypes.sizeof(_abi.KltEpipolarParams) == 28
    assert backend.EPIPOLAR_DTYPE == EPIPOLAR_DTYPE and backend.EPIPOLAR_DTYPE.itemsize == 96
    assert [f[0] for f in _abi.KltEpipolarModel._fields_] == list(EPIPOLAR_DTYPE.names)
    assert [getattr(_abi.KltEpipolarModel, k).offset for k in EPIPOLAR_DTYPE.names] == [EPIPOLAR_DTYPE.fields[k][1] for k in EPIPOLAR_DTYPE.names]
    lib.klt_abi_version.restype = ctypes.c_int
    assert lib.klt_abi_version() == 11                       # additive: the version stays


def test_the_host_entry_point_refuses_null_and_empty_records():
    from pyfeaturetrack_amd import _abi
    lib = _abi.load_library()
    F = (ctypes.c_double * 9)()
    rec = _abi.KltEpipolarModel()
    assert lib.klt_epipolar_matrix(None, F) == -1 and lib.klt_epipolar_matrix(ctypes.byref(rec), None) == -1
    assert lib.klt_epipolar_matrix(ctypes.byref(rec), F) == -3               # valid == 0
    rec.valid, rec.pad = 1, 320 | 240 << 16
    assert lib.klt_epipolar_matrix(ctypes.byref(rec), F) == -3               # f all zero: no direction
    rec.f[5], rec.f[7] = -1.0, 1.0                                           # a sideways step: F = [e1]x
    assert lib.klt_epipolar_matrix(ctypes.byref(rec), F) == 0
    got = np.array(F).reshape(3, 3)
    assert np.allclose(got * np.sqrt(2.0), [[0, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-15)
