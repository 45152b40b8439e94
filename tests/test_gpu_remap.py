"""The remap ingest stage on the device (include/klt_gpu.h, "Remap ingest stage") against its rule in numpy
(tests/remap_expected.py), byte for byte: the kernel by name (klt_remap_u8), and through a slot -- every plane of the three pyramids a
context with a map builds equals the plane a map-less context builds from the rule's output, for every level-0 kernel, adopted frames,
batches, map changes, swaps, refusals and the selection on the raw frame; and both ingest stages together."""
import ctypes as C
import os

import numpy as np
import pytest

import equalize_expected as ee
import remap_expected as re_
from conftest import GOLDEN, read_pgm
from helpers import make_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, first_difference

pytestmark = pytest.mark.gpu
OPT_L0_LAZY_GRAD, OPT_L0_LEAN_FORM, OPT_FAIL_ALLOC_AFTER = 22, 23, 19
ERR_ARG, ERR_STATE = "error -1:", "error -3:"
LEVELS, SS = 2, 4


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """the context with no map that builds from the rule's output"""
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def img0():
    return read_pgm(os.path.join(GOLDEN, "img0.pgm"))


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if bad.size:
        y, x = divmod(int(bad[0]), got.shape[1])
        raise AssertionError("%s: %d of %d bytes differ; first at (x %d, y %d): %d, the rule says %d" %
                             (what, bad.size, got.size, x, y, got[y, x], want[y, x]))


def _remap(ctx, frame, pitch=None):
    """klt_remap_u8 under the context's map; a pitch above the width: the padding holds bytes that must not count"""
    nrows, ncols = frame.shape
    if pitch is None or pitch == ncols:
        return ctx.remap(frame)
    wide = np.full((nrows, pitch), 0xA5, np.uint8)
    wide[:, :ncols] = frame
    return ctx.remap(wide, ncols=ncols)


# ------------------------------------------------------------------------------------------------- (a) the kernel by name
# (ncols, nrows, pitch): narrower than one lane's piece, widths off every multiple of 4, 16 and 64, fewer rows than a tile, padded rows
SHAPES = [(1, 1, 1), (3, 2, 3), (4, 4, 4), (5, 3, 5), (17, 33, 17), (67, 45, 80), (64, 48, 64), (130, 70, 130), (257, 9, 260)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_p%d" % s)
def test_kernel_equals_the_rule(ctx, shape):
    ncols, nrows, pitch = shape
    frames = (("random", re_.random_frame(ncols, nrows, 3)), ("constant", re_.constant_frame(ncols, nrows)),
              ("two-level", re_.two_level_frame(ncols, nrows)))
    try:
        for name, make in re_.MAPS.items():
            mx, my = make(ncols, nrows)
            ctx.set_remap(mx, my)
            for kind, frame in frames:
                _same_bytes(_remap(ctx, frame, pitch), re_.remap(frame, mx, my), "%s map, %s frame" % (name, kind))
    finally:
        ctx.set_remap()


def test_kernel_seeded_draws(ctx):
    try:
        for seed in range(40):
            frame, (mx, my), pitch, name = re_.trial(seed)
            ctx.set_remap(mx, my)
            _same_bytes(_remap(ctx, frame, pitch), re_.remap(frame, mx, my),
                        "draw %d: %d x %d, pitch %d, %s map" % (seed, frame.shape[1], frame.shape[0], pitch, name))
    finally:
        ctx.set_remap()


def test_kernel_refusals(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError
    frame = re_.random_frame(20, 10, 1)
    ctx.set_remap()
    with pytest.raises(KltBackendError, match=ERR_STATE):          # no map set
        ctx.remap(frame)
    mx, my = re_.rotation_map(20, 10)
    try:
        ctx.set_remap(mx, my)
        with pytest.raises(KltBackendError, match=ERR_ARG + ".*19 by 10.*20 by 10"):
            ctx.remap(frame[:, :19])
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.remap(frame[:9])
        lib, h = ctx._lib, ctx._h
        one = np.zeros((1, 1), np.int32)
        assert lib.klt_set_remap(h, one.ctypes.data, None, 1, 1) == -1                     # one plane only
        assert lib.klt_set_remap(h, one.ctypes.data, one.ctypes.data, 0, 1) == -1          # sizes in 1 .. 65535
        assert lib.klt_set_remap(h, one.ctypes.data, one.ctypes.data, 1, 65536) == -1
        _same_bytes(ctx.remap(frame), re_.remap(frame, mx, my), "the context after the refusals")      # (the map it had)
    finally:
        ctx.set_remap()


# ------------------------------------------------------------------------------------------------------ (b) through a slot
def _planes(c, slot, levels=LEVELS):
    return [c.download_level(slot, p, l) for l in range(levels) for p in range(3)]


def _same_planes(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        bad = first_difference(a, b)
        assert not bad, "%s: plane %d of level %d: %s" % (what, i % 3, i // 3, bad)


# name -> (options, (ncols, nrows), frames, klt_level0_path code): the cases of tests/test_gpu_equalize.py
PATHS = {
    "two-pass": ({OPT_FUSED_KERNELS: 0}, (203, 165), 2, 0),
    "rb 16-row": ({}, (180, 200), 2, 2),
    "rb 32-row": ({OPT_FUSED_HREDUCE: 0, OPT_L0_STREAM: 0}, (640, 480), 4, 3),
    "rb 32-row + reduction": ({OPT_L0_STREAM: 0}, (640, 480), 16, 4),
    "stream 64": ({OPT_L0_STREAM: 1, OPT_L0_LAZY_GRAD: 0}, (256, 2560), MAX_BATCH, 6),
    "stream 128": ({OPT_L0_STREAM: 2, OPT_L0_LAZY_GRAD: 0}, (256, 4096), MAX_BATCH, 8),
    "lean 64": ({OPT_L0_STREAM: 1, OPT_L0_LAZY_GRAD: 2}, (256, 2560), MAX_BATCH, 6),
    "lean 128 banded": ({OPT_L0_STREAM: 2, OPT_L0_LAZY_GRAD: 2, OPT_L0_LEAN_FORM: 0}, (256, 4096), MAX_BATCH, 8),
    "lean 128 wave": ({OPT_L0_STREAM: 2, OPT_L0_LAZY_GRAD: 2, OPT_L0_LEAN_FORM: 1}, (256, 4096), MAX_BATCH, 8),
}
DEFAULTS = {OPT_FUSED_KERNELS: 1, OPT_FUSED_HREDUCE: 1, OPT_L0_STREAM: 2, OPT_L0_LAZY_GRAD: 1, OPT_L0_LEAN_FORM: 1}


@pytest.mark.parametrize("path", list(PATHS))
def test_slot_build_equals_build_from_the_rule(ctx, plain, path):
    options, (ncols, nrows), count, code = PATHS[path]
    raw = [re_.textured_frame(ncols, nrows, k + 1) for k in range(2)]
    mx, my = re_.rotation_map(ncols, nrows, 9.0)
    want = [re_.remap(f, mx, my) for f in raw]
    tc = make_tc(levels=LEVELS, ss=SS)
    look = sorted({0, 1, count - 1})
    try:
        for c, frames, on in ((ctx, raw, 1), (plain, want, 0)):
            c.configure(tc)
            if on:
                c.set_remap(mx, my)
            for opt, value in options.items():
                c.set_option(opt, value)
            for k in range(count):
                c.upload(k, frames[k % 2])
            c.build_pyramids_batch(list(range(count)), sync=True)
            assert c.level0_path()[0] == code, "%s: klt_level0_path says %d, the case was written for %d" % (path, c.level0_path()[0], code)
            assert c.level0_lean() == (options.get(OPT_L0_LAZY_GRAD) == 2)
            assert c.remap_path() == on
        for k in look:
            _same_bytes(ctx.download_remapped(k, ncols, nrows), want[k % 2], "%s: klt_download_remapped_u8 of slot %d" % (path, k))
            _same_planes(_planes(ctx, k), _planes(plain, k), "%s, slot %d" % (path, k))
        from pyfeaturetrack_amd._abi import KltBackendError
        with pytest.raises(KltBackendError, match=ERR_STATE):
            plain.download_remapped(0, ncols, nrows)
        # the slots' remapped frames are still valid: a rebuild enqueues no remap launch and gives the same planes
        ctx.build_pyramids_batch(list(range(count)), sync=True)
        assert ctx.remap_path() == 0
        _same_planes(_planes(ctx, look[-1]), _planes(plain, look[-1]), "%s, rebuilt slot %d" % (path, look[-1]))
    finally:
        for c in (ctx, plain):
            for opt, value in DEFAULTS.items():
                c.set_option(opt, value)
            c.set_remap()
            for k in range(2, count):
                c.slot_free(k)


def test_adopted_frame_is_read_and_never_written(ctx, plain, img0):
    img1 = read_pgm(os.path.join(GOLDEN, "img1.pgm"))
    raw = [img0, img1]
    mx, my = re_.barrel_map(320, 240)
    want = [re_.remap(f, mx, my) for f in raw]
    tc = make_tc()
    both = np.concatenate([raw[0].ravel(), raw[1].ravel()])
    dev = ctx.device_alloc(both.nbytes + 64)
    try:
        ctx.device_write(dev, np.concatenate([both, np.full(64, 0x5A, np.uint8)]))
        ctx.configure(tc)
        ctx.set_remap(mx, my)
        plain.configure(tc)
        for k in range(2):
            ctx.adopt_u8(k, dev + k * raw[0].size, 320, 240)
            plain.upload(k, want[k])
        ctx.build_pyramids_batch([0, 1], sync=True)
        plain.build_pyramids_batch([0, 1], sync=True)
        assert ctx.remap_path() == 1 and plain.remap_path() == 0
        for k in range(2):
            _same_bytes(ctx.download_remapped(k, 320, 240), want[k], "adopted slot %d" % k)
            _same_planes(_planes(ctx, k, tc.nPyramidLevels), _planes(plain, k, tc.nPyramidLevels), "adopted slot %d" % k)
        got, placed = ctx.select(0, 100, use_pyramid=True)
        exp, placed_exp = plain.select(0, 100, use_pyramid=True)
        assert placed == placed_exp and got.tobytes() == exp.tobytes()
        raw_sel, _ = ctx.select(0, 100, use_pyramid=False)
        raw_exp, _ = plain.select(0, 100, use_pyramid=False)
        assert raw_sel.tobytes() == raw_exp.tobytes()
        out, tracked = ctx.track(0, 1, got)
        out_exp, tracked_exp = plain.track(0, 1, exp)
        assert tracked == tracked_exp and out.tobytes() == out_exp.tobytes()
        # the caller's buffer, and the guard bytes behind it, as they were
        ctx.sync()
        back = np.zeros(both.nbytes + 64, np.uint8)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(back.ctypes.data, dev, back.nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert np.array_equal(back[:both.nbytes], both) and (back[both.nbytes:] == 0x5A).all()
    finally:
        ctx.set_remap()
        for k in range(2):
            ctx.slot_free(k)
        ctx.device_free(dev)


@pytest.mark.parametrize("size", [(67, 45), (320, 240)], ids=lambda s: "%dx%d" % s)
def test_batch_map_change_and_swap(ctx, plain, img0, size):
    """a batch of same-size frames in one launch; one slot of another size refuses the whole batch; a new map voids the copies, the
    first map again gives the first bytes again; swapped slots take their remapped frames along"""
    from pyfeaturetrack_amd._abi import KltBackendError
    ncols, nrows = size
    tc = make_tc(levels=LEVELS, ss=SS)
    raw = [img0 if size == (320, 240) else re_.textured_frame(ncols, nrows, 1)] + [re_.textured_frame(ncols, nrows, k) for k in (2, 3)]
    maps = [re_.rotation_map(ncols, nrows, 11.0), re_.barrel_map(ncols, nrows)]
    other = re_.textured_frame(ncols + 4, nrows, 9)
    try:
        ctx.configure(tc)
        plain.configure(tc)
        ctx.set_remap(*maps[0])
        for k in range(3):
            ctx.upload(k, raw[k])
        # a slot of another size in the batch: KLT_ERR_ARG naming both sizes, nothing enqueued, no slot got a remapped frame
        ctx.upload(3, other)
        ctx.timing_enable(True)
        with pytest.raises(KltBackendError, match=ERR_ARG + ".*%d by %d.*%d by %d" % (ncols + 4, nrows, ncols, nrows)):
            ctx.build_pyramids_batch([0, 1, 3, 2], sync=True)
        assert sum(t["launches"] for t in ctx.timing_read()) == 0
        for k in range(3):
            with pytest.raises(KltBackendError, match=ERR_STATE):
                ctx.download_remapped(k, ncols, nrows)
        # ... and the context still builds: the three frames of the map's size in ONE remap launch
        ctx.build_pyramids_batch([0, 1, 2], sync=True)
        times = {t["name"]: t["launches"] for t in ctx.timing_read()}
        ctx.timing_enable(False)
        assert times.get("remap") == 1, times
        assert ctx.remap_path() == 1
        for which in (0, 1, 0):
            ctx.set_remap(*maps[which])                            # (a new map, also the first one again: every copy is void)
            with pytest.raises(KltBackendError, match=ERR_STATE):
                ctx.download_remapped(0, ncols, nrows)
            ctx.build_pyramids_batch([0, 1, 2], sync=True)
            assert ctx.remap_path() == 1
            want = [re_.remap(f, *maps[which]) for f in raw]
            for k in range(3):
                plain.upload(k, want[k])
            plain.build_pyramids_batch([0, 1, 2], sync=True)
            for k in range(3):
                _same_bytes(ctx.download_remapped(k, ncols, nrows), want[k], "map %d, slot %d" % (which, k))
                _same_planes(_planes(ctx, k), _planes(plain, k), "map %d, slot %d" % (which, k))
        # one new frame: only its slot is remapped again; swapped slots take their remapped frames along
        ctx.upload(1, raw[2])
        ctx.swap_slots(0, 2)
        ctx.timing_enable(True)
        ctx.build_pyramids_batch([0, 1, 2], sync=True)
        times = {t["name"]: t["launches"] for t in ctx.timing_read()}
        ctx.timing_enable(False)
        assert ctx.remap_path() == 1 and times.get("remap") == 1
        for k, src in enumerate((2, 2, 0)):
            _same_bytes(ctx.download_remapped(k, ncols, nrows), want[src], "slot %d after the swap" % k)
            _same_planes(_planes(ctx, k), _planes(plain, src), "slot %d after the swap" % k)
    finally:
        ctx.timing_enable(False)
        ctx.set_remap()
        for c in (ctx, plain):
            for k in range(4):
                c.slot_free(k)


def test_refusals_leave_the_slot_usable(ctx, plain, img0):
    from pyfeaturetrack_amd._abi import KltBackendError, KltOutOfMemory
    tc = make_tc()
    levels = tc.nPyramidLevels
    small = re_.textured_frame(67, 45, 2)
    big_map, small_map = re_.barrel_map(320, 240), re_.rotation_map(67, 45)
    try:
        ctx.configure(tc)
        plain.configure(tc)
        # an f32 slot
        ctx.set_remap(*big_map)
        ctx.upload(0, img0.astype(np.float32))
        with pytest.raises(KltBackendError, match="error -3: remapping takes 8-bit frames"):
            ctx.build_pyramids(0, sync=True)
        with pytest.raises(KltBackendError, match="error -3: remapping takes 8-bit frames"):
            ctx.select(0, 10, use_pyramid=False)
        ctx.set_remap()
        ctx.build_pyramids(0, sync=True)
        plain.upload(0, img0.astype(np.float32))
        plain.build_pyramids(0, sync=True)
        _same_planes(_planes(ctx, 0, levels), _planes(plain, 0, levels), "the f32 slot with no map")
        # a frame of another size than the map's, built and selected on
        one = make_tc(levels=1, ss=2)
        ctx.configure(one)                                         # (a tracking context's own switch is off: the map goes after it)
        plain.configure(one)
        ctx.set_remap(*big_map)
        ctx.upload(1, small)
        with pytest.raises(KltBackendError, match=ERR_ARG + ".*67 by 45.*320 by 240"):
            ctx.build_pyramids(1, sync=True)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.select(1, 10, use_pyramid=False)
        # the allocation of the slot's remapped frame fails: KLT_ERR_NOMEM, and the next build has it
        ctx.set_remap()
        ctx.build_pyramids(1, sync=True)                           # (everything else the build allocates is there now)
        ctx.set_remap(*small_map)
        ctx.set_option(OPT_FAIL_ALLOC_AFTER, 0)
        try:
            with pytest.raises(KltOutOfMemory):
                ctx.build_pyramids(1, sync=True)
        finally:
            ctx.set_option(OPT_FAIL_ALLOC_AFTER, -1)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.download_remapped(1, 67, 45)
        ctx.build_pyramids(1, sync=True)
        want = re_.remap(small, *small_map)
        _same_bytes(ctx.download_remapped(1, 67, 45), want, "the slot after the failed allocation")
        plain.upload(1, want)
        plain.build_pyramids(1, sync=True)
        _same_planes(_planes(ctx, 1, 1), _planes(plain, 1, 1), "the slot after the failed allocation")
        ctx.set_remap()
        ctx.build_pyramids(1, sync=True)
        assert ctx.remap_path() == 0
        plain.upload(1, small)
        plain.build_pyramids(1, sync=True)
        _same_planes(_planes(ctx, 1, 1), _planes(plain, 1, 1), "that slot with no map")
    finally:
        ctx.set_option(OPT_FAIL_ALLOC_AFTER, -1)
        ctx.set_remap()
        for c in (ctx, plain):
            for k in range(2):
                c.slot_free(k)


@pytest.mark.parametrize("smooth", [True, False], ids=["smoothed", "unsmoothed"])
@pytest.mark.parametrize("size", [(67, 45), (320, 240)], ids=lambda s: "%dx%d" % s)
def test_selection_on_the_raw_frame(ctx, plain, img0, size, smooth):
    ncols, nrows = size
    # (the default border leaves no candidate in a 67 x 45 frame: one level and a 3 x 3 window there)
    tc = make_tc(smoothBeforeSelecting=smooth) if size == (320, 240) else make_tc(levels=1, ss=2, window=3, smoothBeforeSelecting=smooth)
    frame = img0 if size == (320, 240) else re_.textured_frame(ncols, nrows, 4)
    mx, my = re_.rotation_map(ncols, nrows, 7.0)
    want = re_.remap(frame, mx, my)
    try:
        ctx.configure(tc)
        ctx.set_remap(mx, my)
        plain.configure(tc)
        ctx.upload(0, frame)                                       # a fresh upload: the selection finds the remapped frame stale
        plain.upload(0, want)
        got, placed = ctx.select(0, 60, use_pyramid=False)
        exp, placed_exp = plain.select(0, 60, use_pyramid=False)
        assert placed == placed_exp and placed > 0 and got.tobytes() == exp.tobytes()
        _same_bytes(ctx.download_remapped(0, ncols, nrows), want, "the frame the selection read")
    finally:
        ctx.set_remap()
        ctx.slot_free(0)
        plain.slot_free(0)


def test_no_map_reports_path_0(plain, img0):
    plain.configure(make_tc())
    plain.upload(0, img0)
    plain.build_pyramids(0, sync=True)
    assert plain.remap_path() == 0
    plain.slot_free(0)


# ------------------------------------------------------------------------------------------------ (c) both ingest stages on
@pytest.mark.parametrize("size", [(67, 45), (320, 240)], ids=lambda s: "%dx%d" % s)
def test_remap_then_clahe(ctx, plain, img0, size):
    ncols, nrows = size
    tc = make_tc(levels=LEVELS, ss=SS)
    frame = ee.darken_left_half(img0) if size == (320, 240) else ee.darken_left_half(re_.textured_frame(ncols, nrows, 6))
    mx, my = re_.barrel_map(ncols, nrows)
    tiles = (8, 8) if size == (320, 240) else (3, 2)
    q8 = 768
    remapped = re_.remap(frame, mx, my)
    both = ee.clahe(remapped, tiles[0], tiles[1], q8)
    try:
        ctx.configure(tc)
        plain.configure(tc)
        ctx.set_remap(mx, my)
        ctx.set_equalize_params(mode=1, tiles_x=tiles[0], tiles_y=tiles[1], clip_q8=q8)
        ctx.upload(0, frame)
        ctx.build_pyramids(0, sync=True)
        assert ctx.remap_path() == 1 and ctx.equalize_path() == 1
        _same_bytes(ctx.download_remapped(0, ncols, nrows), remapped, "the remapped frame")
        _same_bytes(ctx.download_equalized(0, ncols, nrows), both, "the equalised remapped frame")
        plain.upload(0, both)
        plain.build_pyramids(0, sync=True)
        _same_planes(_planes(ctx, 0), _planes(plain, 0), "remap, then CLAHE")
        # the selection on the raw frame reads the same chain (a fresh upload: both copies stale)
        ctx.upload(0, frame)
        got, _ = ctx.select(0, 40, use_pyramid=False)
        exp, _ = plain.select(0, 40, use_pyramid=False)
        assert got.tobytes() == exp.tobytes()
        # new equalisation parameters alone: the remapped frame stays, the equalised one is made again
        ctx.set_equalize_params(mode=1, tiles_x=tiles[0], tiles_y=tiles[1], clip_q8=0)
        ctx.build_pyramids(0, sync=True)
        assert ctx.remap_path() == 0 and ctx.equalize_path() == 1
        _same_bytes(ctx.download_equalized(0, ncols, nrows), ee.clahe(remapped, tiles[0], tiles[1], 0), "new clip limit")
        # remap off again: the equalised frame is the one of the frame as it came
        ctx.set_equalize_params(mode=1, tiles_x=tiles[0], tiles_y=tiles[1], clip_q8=q8)
        ctx.set_remap()
        ctx.build_pyramids(0, sync=True)
        assert ctx.remap_path() == 0 and ctx.equalize_path() == 1
        plainly = ee.clahe(frame, tiles[0], tiles[1], q8)
        _same_bytes(ctx.download_equalized(0, ncols, nrows), plainly, "CLAHE alone")
        plain.upload(0, plainly)
        plain.build_pyramids(0, sync=True)
        _same_planes(_planes(ctx, 0), _planes(plain, 0), "CLAHE alone")
    finally:
        ctx.set_remap()
        ctx.set_equalize_params()
        ctx.slot_free(0)
        plain.slot_free(0)
