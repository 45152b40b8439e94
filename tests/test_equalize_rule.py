"""The CLAHE ingest stage's rule (include/klt_gpu.h; tests/equalize_expected.py restates it in numpy) without a device: hand-worked
cases, the properties that hold for every equalisable shape, tc.equalization's parameters, and what the stage is for -- the CPU oracle
finds the corners of a darkened half again on the equalised frame."""
import os
import types

import numpy as np
import pytest

import equalize_expected as ee
from conftest import GOLDEN, read_pgm
from pyfeaturetrack_amd.klt import KLT_TrackingContext
from pyfeaturetrack_amd.params import equalisable, equalization_for_frames, equalize_params_from_tc, params_from_tc

# (ncols, nrows, tiles_x, tiles_y, clip_q8): the shape table of tests/test_gpu_equalize.py -- every row is equalisable
SHAPES = [(64, 48, 8, 8, 768), (67, 45, 3, 2, 768), (33, 17, 4, 3, 1), (5, 3, 5, 3, 768), (4, 4, 1, 1, 0), (130, 70, 64, 64, 768),
          (320, 240, 8, 8, 768), (320, 240, 8, 8, 10240)]


# --------------------------------------------------------------------------------------------------------------- hand-worked
FOUR = np.array([[0, 0, 1, 1], [2, 2, 3, 3], [0, 1, 2, 3], [3, 3, 3, 3]], np.uint8)      # bins 0, 1, 2: 3 pixels each; bin 3: 7


def test_one_tile_without_clipping():
    # cdf 3, 6, 9, 16; lut = (cdf * 255 + 8) // 16 = 48, 96, 143, 255; one tile: D = 1 on both axes, the pixel is its LUT entry
    lut = ee.tile_lut(FOUR, 0)
    assert lut[:4].tolist() == [48, 96, 143, 255] and (lut[3:] == 255).all()
    want = np.array([48, 96, 143, 255], np.uint8)[FOUR]
    assert np.array_equal(ee.clahe(FOUR, 1, 1, 0), want)


def test_one_tile_with_clipping():
    # clip limit 2.0: cap = max(1, (512 * 16) >> 16) = 1; excess = 2 + 2 + 2 + 6 = 12; every bin gets 12 // 256 = 0, and the bins
    # (k * 256) // 12, k = 0 .. 11 = 0, 21, 42, 64, 85, 106, 128, 149, 170, 192, 213, 234 one more each
    h = ee.redistributed_histogram(FOUR, 512)
    assert h[:4].tolist() == [2, 1, 1, 1] and h.sum() == 16
    assert np.flatnonzero(h[4:]).tolist() == [b - 4 for b in (21, 42, 64, 85, 106, 128, 149, 170, 192, 213, 234)]
    # cdf 2, 3, 4, 5 -> (cdf * 255 + 8) // 16 = 32, 48, 64, 80
    assert ee.tile_lut(FOUR, 512)[:4].tolist() == [32, 48, 64, 80]
    assert np.array_equal(ee.clahe(FOUR, 1, 1, 512), np.array([32, 48, 64, 80], np.uint8)[FOUR])


def test_two_tiles_pin_the_interpolation_weights():
    # 8 columns, 2 tiles: edges 0, 4, 8; centres C_0 = 4, C_1 = 12; P = 2x + 1 = 1, 3 | 5, 7, 9, 11 | 13, 15
    first, second, w, d = ee.axis_weights(8, 2)
    assert first.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and second.tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert w.tolist() == [0, 0, 1, 3, 5, 7, 0, 0] and d.tolist() == [1, 1, 8, 8, 8, 8, 1, 1]
    # one tile on the other axis: D is always 1
    assert [a.tolist() for a in ee.axis_weights(3, 1)] == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 1, 1]]
    # left tile all 10, right tile all 200: lut0 = 0 below 10 and 255 from 10 on, lut1 = 0 below 200 and 255 from 200 on
    frame = np.array([[10, 10, 10, 10, 200, 200, 200, 200]] * 2, np.uint8)
    # column 2: (255 * 7 + 0 * 1 + 4) // 8 = 223; column 3: (255 * 5 + 0 * 3 + 4) // 8 = 159; columns 4, 5: both LUTs give 255
    assert ee.clahe(frame, 2, 1, 0).tolist() == [[255, 255, 223, 159, 255, 255, 255, 255]] * 2


def test_one_pixel_tiles_map_to_255():
    assert (ee.clahe(np.arange(15, dtype=np.uint8).reshape(3, 5), 5, 3, 768) == 255).all()


# ---------------------------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d_%d" % s)
def test_properties_of_every_shape(shape):
    ncols, nrows, tx, ty, clip_q8 = shape
    assert ee.equalisable(ncols, nrows, tx, ty) and equalisable(ncols, nrows, tx, ty)
    xe, ye = ee.edges(ncols, tx), ee.edges(nrows, ty)
    assert xe[0] == 0 and xe[-1] == ncols and np.diff(xe).min() >= 1 and np.diff(xe).max() - np.diff(xe).min() <= 1
    for frame in (ee.random_frame(ncols, nrows, 3), ee.two_bin_frame(ncols, nrows), ee.constant_frame(ncols, nrows)):
        for j in range(ty):
            for i in range(tx):
                tile = frame[ye[j]:ye[j + 1], xe[i]:xe[i + 1]]
                assert ee.redistributed_histogram(tile, clip_q8).sum() == tile.size      # the bins still sum to the area
        lut = ee.luts(frame, tx, ty, clip_q8)
        assert (np.diff(lut, axis=2) >= 0).all() and (lut[:, :, 255] == 255).all() and lut.min() >= 0
        out = ee.clahe(frame, tx, ty, clip_q8)
        assert out.dtype == np.uint8 and out.shape == frame.shape


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d_%d" % s)
def test_a_constant_frame_stays_constant(shape):
    """Where the rule makes it so: every tile's LUT is a function of the tile's area alone on a constant frame, so the frame stays constant
    when all tiles have one area -- and, whatever the areas, without clipping (cdf[v] = A in every tile: 255 everywhere).  With clipping
    and tiles that differ by a pixel the LUT entries differ by their rounding and so does the frame: 33 x 17 in 4 x 3 tiles with cap 1
    (areas 40, 45, 48, 54) comes out as 83 .. 85, 130 x 70 in 64 x 64 tiles (areas 2, 3, 4, 6) likewise over several levels.  That is the
    rule as the header states it, not an error of a restatement: those rows are held to the bound below instead."""
    ncols, nrows, tx, ty, clip_q8 = shape
    flat = ee.constant_frame(ncols, nrows)
    assert (ee.clahe(flat, tx, ty, 0) == 255).all()
    areas = {int(w) * int(h) for w in np.diff(ee.edges(ncols, tx)) for h in np.diff(ee.edges(nrows, ty))}
    out = ee.clahe(flat, tx, ty, clip_q8)
    if len(areas) == 1 or clip_q8 == 0:
        assert len(np.unique(out)) == 1
    else:
        # an interpolated pixel lies between the LUT entries it mixes: the frame stays within the spread of the tiles' entries for 77
        entries = ee.luts(flat, tx, ty, clip_q8)[:, :, 77]
        assert entries.min() <= out.min() and out.max() <= entries.max()
    assert len(np.unique(ee.clahe(ee.constant_frame(64, 48), 8, 8, 768))) == 1 and len(np.unique(ee.clahe(ee.constant_frame(320, 240), 8, 8, 10240))) == 1


def test_the_shape_test():
    assert not ee.equalisable(20, 10, 64, 64) and not equalisable(20, 10, 64, 64)      # more tiles than pixels
    assert ee.equalisable(3840, 2160, 2, 2) and ee.equalisable(3840, 2160, 1, 1) and ee.equalisable(3840, 2160, 8, 8)
    # two tiles across 65535 x 65535: Dx * Dy * 255 = 65535^2 * 255 is no 32-bit number
    assert not ee.equalisable(65535, 65535, 2, 2) and not equalisable(65535, 65535, 2, 2)
    for seed in range(40):
        frame, tx, ty, clip_q8, pitch = ee.trial(seed)
        assert equalisable(frame.shape[1], frame.shape[0], tx, ty) and pitch >= frame.shape[1] and 0 <= clip_q8 <= 1 << 20


# ---------------------------------------------------------------------------------------------------------------- parameters
def test_defaults():
    tc = KLT_TrackingContext()
    assert tc.equalization is None and tuple(tc.clahe_tiles) == (8, 8) and tc.clahe_clip_limit == 3.0
    eq = equalize_params_from_tc(tc)
    assert (eq.mode, eq.tiles_x, eq.tiles_y, eq.clip_q8) == (0, 8, 8, 768)
    bare = types.SimpleNamespace()                           # a tracking context made elsewhere has none of the three
    eq = equalize_params_from_tc(bare)
    assert (eq.mode, eq.tiles_x, eq.tiles_y, eq.clip_q8) == (0, 8, 8, 768)
    tc.equalization, tc.clahe_tiles, tc.clahe_clip_limit = "clahe", (3, 2), 40.0
    eq = equalize_params_from_tc(tc)
    assert (eq.mode, eq.tiles_x, eq.tiles_y, eq.clip_q8) == (1, 3, 2, 10240) and ee.clip_q8_of(40.0) == 10240
    for off in (None, 0, 0.0):
        tc.clahe_clip_limit = off
        assert equalize_params_from_tc(tc).clip_q8 == 0 and ee.clip_q8_of(off) == 0
    tc.clahe_clip_limit = 4096
    assert equalize_params_from_tc(tc).clip_q8 == 1 << 20


@pytest.mark.parametrize("field,value", [("equalization", "CLAHE"), ("equalization", True), ("equalization", 1), ("equalization", "he"),
                                         ("clahe_tiles", (0, 8)), ("clahe_tiles", (8, 65)), ("clahe_tiles", (8,)), ("clahe_tiles", 8),
                                         ("clahe_tiles", (8.0, 8)), ("clahe_tiles", (True, 8)), ("clahe_tiles", "88"),
                                         ("clahe_tiles", (8, 8, 8)), ("clahe_clip_limit", -1.0), ("clahe_clip_limit", float("nan")),
                                         ("clahe_clip_limit", float("inf")), ("clahe_clip_limit", 4096.5), ("clahe_clip_limit", "3")])
def test_refusals(field, value):
    tc = KLT_TrackingContext()
    tc.equalization = "clahe"
    setattr(tc, field, value)
    with pytest.raises(ValueError, match="tc." + field):
        equalize_params_from_tc(tc)


def test_frames_the_switch_does_not_take():
    tc = KLT_TrackingContext()
    u8, f32, rgb = np.zeros((48, 64), np.uint8), np.zeros((48, 64), np.float32), np.zeros((48, 64, 3), np.uint8)
    for img in (u8, f32, rgb):
        assert equalization_for_frames(tc, img).mode == 0            # switched off: any frame
    tc.equalization = "clahe"
    assert equalization_for_frames(tc, u8, u8).mode == 1
    for img in (f32, rgb):
        with pytest.raises(ValueError, match="tc.equalization"):
            equalization_for_frames(tc, u8, img)
    tc.clahe_tiles = (64, 64)
    with pytest.raises(ValueError, match="tc.equalization"):
        equalization_for_frames(tc, u8)                              # 48 rows, 64 tiles down


# --------------------------------------------------------------------------------------------------------------- what it is for
def test_selection_finds_the_dark_half_again():
    """tests/golden/img0.pgm with its left half darkened to v * 0.08 + 5: the oracle's selection of 300 features puts 149 in the left half
    of the untouched frame, 92 in that of the darkened one and 142 in that of the darkened frame equalised (8 x 8 tiles, clip limit 3.0)"""
    from oracle import klt_oracle as ko
    img = read_pgm(os.path.join(GOLDEN, "img0.pgm"))
    dark = ee.darken_left_half(img)
    p = params_from_tc(KLT_TrackingContext())
    half = img.shape[1] // 2

    def left(frame):
        fl = ko.select_good_features(p, frame.astype(np.float32), 300)
        return int(((fl["val"] >= 0) & (fl["x"] < half)).sum())
    plain, darkened, equalised = left(img), left(dark), left(ee.clahe(dark, 8, 8, 768))
    print("left-half features: untouched %d, darkened %d, darkened then equalised %d" % (plain, darkened, equalised))
    assert equalised > darkened
    assert abs(equalised - plain) <= 10
