"""The remap ingest stage's rule (tests/remap_expected.py; include/klt_gpu.h, "Remap ingest stage") and its host
side in pyfeaturetrack_amd.params -- no GPU: a hand-worked case, the identities the rule promises, KLTUndistortMap against an independent
scalar evaluation of the lens model, the mask, the source positions, the table object, the refusals; and what the stage is for, with the
homography check's numpy rule (tests/homography_expected.py): static points under a pan seen through a barrel lens."""
import math
import types

import numpy as np
import pytest

import homography_expected as he
import remap_expected as re_
from pyfeaturetrack_amd.params import (KLT_RemapTable, KLTCreateRemap, KLTRemapSourcePositions, KLTRemapValidMask, KLTUndistortMap,
                                       remap_for_frames, remap_from_tc)

I32 = np.int32


def test_hand_worked_3x3():
    """f[y][x] = 30 y + 10 x is linear, so inside the frame the rule gives floor((30 Y + 10 X) / 256 + 1 / 2) (the weights sum to 65536)"""
    frame = np.array([[0, 10, 20], [30, 40, 50], [60, 70, 80]], np.uint8)
    mx = np.array([[128, -5, re_.INT32_MAX], [300, 511, 512 + 77], [0, 256, 384]], I32)
    my = np.array([[64, 512, re_.INT32_MIN], [300, 1, 384], [512, 512, 448]], I32)
    # (0,0): (1920 + 1280) / 256 = 12.5 -> 13.   (1,0): X clamps to 0, row 2: 60.   (2,0): X clamps to 512, Y to 0: 20.
    # (0,1): 12000 / 256 = 46.875 -> 47.   (1,1): (30 + 5110) / 256 = 20.08 -> 20.   (2,1): X clamps to 512; 45 + 20 = 65.
    # (0,2): 60.   (1,2): 70.   (2,2): (13440 + 3840) / 256 = 67.5 -> 68.
    want = np.array([[13, 60, 20], [47, 20, 65], [60, 70, 68]], np.uint8)
    assert np.array_equal(re_.remap(frame, mx, my), want)


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (67, 45), (130, 70)])
def test_identity_returns_the_frame(shape):
    frame = re_.random_frame(shape[0], shape[1], 3)
    assert np.array_equal(re_.remap(frame, *re_.identity_map(*shape)), frame)


def test_whole_pixel_shift_replicates_the_edges():
    frame = re_.random_frame(23, 17, 4)
    got = re_.remap(frame, *re_.shift_map(23, 17, 3.0, -2.0))
    want = np.empty_like(frame)
    for y in range(17):
        for x in range(23):
            want[y, x] = frame[min(max(y - 2, 0), 16), min(max(x + 3, 0), 22)]
    assert np.array_equal(got, want)


def test_constant_frame_stays_constant_under_the_wild_map():
    for value in (0, 77, 255):
        frame = re_.constant_frame(67, 45, value)
        assert (re_.remap(frame, *re_.wild_map(67, 45)) == value).all()


def test_int32_extremes_clamp():
    frame = re_.random_frame(9, 7, 5)
    lo, hi = np.full((7, 9), re_.INT32_MIN, I32), np.full((7, 9), re_.INT32_MAX, I32)
    assert (re_.remap(frame, lo, lo) == frame[0, 0]).all()
    assert (re_.remap(frame, hi, hi) == frame[6, 8]).all()
    assert (re_.remap(frame, hi, lo) == frame[0, 8]).all()
    assert (re_.remap(frame, lo, hi) == frame[6, 0]).all()
    # one unit below the last pixel centre still mixes, the centre itself and everything beyond is the edge pixel
    edge = np.full((7, 9), 8 * 256, I32)
    assert (re_.remap(frame, edge, lo) == frame[0, 8]).all() and (re_.remap(frame, edge + 1, lo) == frame[0, 8]).all()


def test_every_map_maker_gives_int32_planes_of_the_frame_shape():
    for name, make in re_.MAPS.items():
        mx, my = make(13, 7)
        assert mx.dtype == I32 and my.dtype == I32 and mx.shape == (7, 13) == my.shape, name
    mx, my = re_.wild_map(67, 45)
    for m in (mx, my):
        assert m.min() == re_.INT32_MIN and m.max() == re_.INT32_MAX and (m < 0).any() and (m > 1 << 24).any()
    for seed in range(6):
        frame, (mx, my), pitch, _ = re_.trial(seed)
        assert frame.shape == mx.shape == my.shape and pitch >= frame.shape[1]


# ----------------------------------------------------------------------------------------------------------------- KLTUndistortMap
K = np.array([[410.0, 0.0, 319.5], [0.0, 405.0, 239.5], [0.0, 0.0, 1.0]])
DIST = (-0.28, 0.09, 0.0011, -0.0007, -0.012)


def _scalar_model(u, v, cam, dist, new_cam):
    """the issue's model, one pixel at a time with Python floats: rectified pixel -> normalised -> distorted -> source pixel"""
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    x, y = (u - new_cam[0][2]) / new_cam[0][0], (v - new_cam[1][2]) / new_cam[1][1]
    r2 = x * x + y * y
    radial = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return cam[0][0] * xd + cam[0][2], cam[1][1] * yd + cam[1][2]


def test_undistort_map_zero_coefficients_is_the_identity():
    for dist in ((0, 0, 0, 0), (0, 0, 0, 0, 0)):
        t = KLTUndistortMap(640, 480, K, dist)
        ix, iy = re_.identity_map(640, 480)
        assert np.array_equal(t.map_x, ix) and np.array_equal(t.map_y, iy)
    t = KLTUndistortMap(640, 480, K, (0, 0, 0, 0), new_camera_matrix=K)
    assert np.array_equal(t.map_x, re_.identity_map(640, 480)[0])


@pytest.mark.parametrize("dist", [DIST, DIST[:4]], ids=["k3", "no_k3"])
def test_undistort_map_equals_the_scalar_model(dist):
    new_cam = np.array([[380.0, 0.0, 322.0], [0.0, 377.0, 236.0], [0.0, 0.0, 1.0]])
    for new in (None, new_cam):
        t = KLTUndistortMap(640, 480, K, dist, new_camera_matrix=new)
        assert t.shape == (480, 640)
        rs = np.random.RandomState(8)
        samples = [(0, 0), (639, 0), (0, 479), (639, 479), (320, 240)] + [(int(rs.randint(640)), int(rs.randint(480))) for _ in range(300)]
        for u, v in samples:
            us, vs = _scalar_model(float(u), float(v), K.tolist(), dist, (K if new is None else new).tolist())
            # 1 unit of 1/256 px: the two evaluations order their FP64 operations differently, and rint may fall either way of a half
            assert abs(int(t.map_x[v, u]) - 256.0 * us) <= 1.0 and abs(int(t.map_y[v, u]) - 256.0 * vs) <= 1.0, (u, v)
            assert abs(int(t.map_x[v, u]) - int(round(256.0 * us))) <= 1 and abs(int(t.map_y[v, u]) - int(round(256.0 * vs))) <= 1, (u, v)


def test_undistort_map_clips_to_int32():
    centred = np.array([[40.0, 0.0, 31.5], [0.0, 40.0, 23.5], [0.0, 0.0, 1.0]])
    t = KLTUndistortMap(64, 48, centred, (1e9, 0, 0, 0))          # (left of the centre far below, right of it far above what 32 bits hold)
    for m in (t.map_x, t.map_y):
        assert m.dtype == I32 and m.min() == re_.INT32_MIN and m.max() == re_.INT32_MAX


def test_source_positions_at_whole_positions_are_the_entries():
    t = KLTUndistortMap(640, 480, K, DIST)
    y, x = np.mgrid[0:480:7, 0:640:9]
    sx, sy = KLTRemapSourcePositions(t, x, y)
    assert np.array_equal(sx, t.map_x[y, x] / 256.0) and np.array_equal(sy, t.map_y[y, x] / 256.0)
    # between four entries: their bilinear mean; outside the frame: the map's edge
    sx, sy = KLTRemapSourcePositions(t, 10.5, 20.5)
    assert sx == pytest.approx(t.map_x[20:22, 10:12].mean() / 256.0, abs=1e-9) and sy == pytest.approx(t.map_y[20:22, 10:12].mean() / 256.0, abs=1e-9)
    sx, sy = KLTRemapSourcePositions(t, -5.0, 1000.0)
    assert sx == t.map_x[479, 0] / 256.0 and sy == t.map_y[479, 0] / 256.0


def test_valid_mask_on_a_hand_made_map():
    # a 4 x 3 frame: x may lie in 0 .. 768, y in 0 .. 512
    mx = np.array([[0, 256, 768, 769], [-1, 255, 512, 768], [256, 256, 256, 256]], I32)
    my = np.array([[0, 0, 0, 0], [256, 256, 256, 256], [-1, 512, 513, 256]], I32)
    t = KLTCreateRemap(mx, my)
    assert np.array_equal(KLTRemapValidMask(t), np.array([[1, 1, 1, 0], [0, 1, 1, 1], [0, 1, 0, 1]], np.uint8))
    # a margin of 1 px: x in 256 .. 512, y in 256 .. 256
    assert np.array_equal(KLTRemapValidMask(t, margin=1), np.array([[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.uint8))
    assert KLTRemapValidMask(t).dtype == np.uint8


def test_table_is_frozen_and_serials_differ():
    mx, my = re_.shift_map(8, 5)
    a, b = KLTCreateRemap(mx, my), KLTCreateRemap(mx, my)
    assert isinstance(a, KLT_RemapTable) and a.serial != b.serial and a.shape == (5, 8)
    assert a.map_x.dtype == I32 and not a.map_x.flags.writeable and not a.map_y.flags.writeable
    with pytest.raises(ValueError):
        a.map_x[0, 0] = 1
    with pytest.raises(AttributeError):
        a.map_x = mx
    with pytest.raises(AttributeError):
        a.serial = 0
    # a copy: the caller's arrays stay the caller's
    mx[0, 0] += 1
    assert a.map_x[0, 0] == mx[0, 0] - 1
    # any integer kind is taken and converted
    c = KLTCreateRemap(mx.astype(np.int64), my.astype(np.int16))
    assert c.map_x.dtype == I32 and c.map_y.dtype == I32 and np.array_equal(c.map_y, my)
    assert KLTUndistortMap(8, 5, K, (0, 0, 0, 0)).serial > c.serial


def test_refusals():
    mx, my = re_.identity_map(8, 5)
    with pytest.raises(TypeError):
        KLTCreateRemap(mx.astype(np.float32), my)
    with pytest.raises(TypeError):
        KLTCreateRemap(mx, my.astype(np.float64))
    with pytest.raises(ValueError):
        KLTCreateRemap(mx, my[:, :7])
    with pytest.raises(ValueError):
        KLTCreateRemap(mx.ravel(), my.ravel())
    with pytest.raises(ValueError):
        KLTCreateRemap(mx.astype(np.int64) + 2 ** 40, my)
    with pytest.raises(ValueError):
        KLTUndistortMap(8, 5, K, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError):
        KLTUndistortMap(0, 5, K, DIST)
    with pytest.raises(ValueError):
        KLTUndistortMap(8, 5, np.eye(2), DIST)
    with pytest.raises(TypeError):
        KLTRemapValidMask((mx, my))
    with pytest.raises(TypeError):
        KLTRemapSourcePositions(mx, 0, 0)
    # the switch on a tracking context: None by default, also where the attribute does not exist; a table; anything else is refused
    table = KLTCreateRemap(mx, my)
    assert remap_from_tc(types.SimpleNamespace()) is None and remap_from_tc(types.SimpleNamespace(remap=None)) is None
    assert remap_from_tc(types.SimpleNamespace(remap=table)) is table
    with pytest.raises(TypeError, match="tc.remap"):
        remap_from_tc(types.SimpleNamespace(remap=(mx, my)))
    tc = types.SimpleNamespace(remap=table)
    frame = re_.random_frame(8, 5, 1)
    assert remap_for_frames(tc, frame, frame) is table and remap_for_frames(types.SimpleNamespace(), frame.astype(np.float32)) is None
    for bad in (frame.astype(np.float32), np.dstack([frame] * 3), frame[:, :7], frame[:4]):
        with pytest.raises(ValueError, match="tc.remap"):
            remap_for_frames(tc, frame, bad)


def test_an_array_without_two_dimensions_is_refused_by_name():
    """a 1-D or 0-D array has no (nrows, ncols) to read: the refusal is the one for a frame that is no single-channel 8-bit image, and
    it says what came instead -- for both ingest stages, which classify a frame with one helper"""
    from pyfeaturetrack_amd.params import equalization_for_frames
    mx, my = re_.identity_map(4, 3)
    remap = types.SimpleNamespace(remap=KLTCreateRemap(mx, my))
    clahe = types.SimpleNamespace(equalization="clahe", clahe_tiles=(1, 1))
    for bad, what in ((np.zeros(12, np.uint8), "a uint8 array of 1 dimensions"), (np.zeros((), np.uint8), "a uint8 array of 0 dimensions"),
                      (np.zeros((3, 4, 1), np.uint8), "a uint8 array of 3 dimensions"), (np.zeros(12, np.float32), "a float32 array of 1 dimensions")):
        with pytest.raises(ValueError, match="tc.remap takes single-channel 8-bit frames .*, not " + what):
            remap_for_frames(remap, bad)
        with pytest.raises(ValueError, match="tc.equalization = 'clahe' takes single-channel 8-bit frames .*, not " + what):
            equalization_for_frames(clahe, bad)


def test_tracking_context_has_the_switch_off():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    assert KLT_TrackingContext().remap is None


# ------------------------------------------------------------------------------------------------------------------- the purpose
LENS_K = np.array([[900.0, 0.0, 959.5], [0.0, 900.0, 539.5], [0.0, 0.0, 1.0]])
LENS_DIST = (-0.12, 0.02, 0.0, 0.0)
RAW_FLAGGED = 62         # of the 383 static points that stay in the frame (DESIGN.md section 9m quotes it)


def lens_scene(npoints=400, seed=3):
    """400 static points in a 1920 x 1080 pinhole frame before and after a pan of 0.04 rad about y (a homography); the raw positions
    are where a barrel lens (LENS_DIST) shows them: the table's source positions of the rectified ones"""
    rs = np.random.RandomState(seed)
    p = np.stack([rs.uniform(60, 1860, npoints), rs.uniform(60, 1020, npoints), np.ones(npoints)])
    a = 0.04
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    q = LENS_K @ R @ np.linalg.inv(LENS_K) @ p
    q = q[:2] / q[2]
    keep = (q[0] >= 60) & (q[0] <= 1860) & (q[1] >= 60) & (q[1] <= 1020)
    return p[0][keep], p[1][keep], q[0][keep], q[1][keep]


def test_homography_check_flags_static_points_through_a_barrel_lens_and_none_once_rectified():
    table = KLTUndistortMap(1920, 1080, LENS_K, LENS_DIST)
    px, py, qx, qy = lens_scene()
    n = len(px)

    def flagged(ax, ay, bx, by):
        fin = he.records(ax, ay, np.arange(n) % 1000, 0)
        fout = he.records(bx, by, he.KLT_TRACKED, 0)
        out, rec = he.homography_check_expected(fin, fout, 1920, 1080)          # the check's defaults: homography_max_error 1 px
        assert int(rec["valid"]) != 0
        return int((out["val"] == he.KLT_HOMOGRAPHY_OUTLIER).sum())

    raw = flagged(*KLTRemapSourcePositions(table, px, py), *KLTRemapSourcePositions(table, qx, qy))
    rectified = flagged(px, py, qx, qy)
    print("homography check on %d static points under a pan: %d flagged in raw coordinates, %d in rectified ones" % (n, raw, rectified))
    assert rectified == 0
    assert raw > 0 and n == 383 and raw == RAW_FLAGGED
