"""The CLAHE ingest stage on the device (include/klt_gpu.h, "CLAHE ingest stage") against its rule in numpy
(tests/equalize_expected.py), byte for byte: the kernel pair by name (klt_equalize_u8), and through a slot -- every plane of the three
pyramids a context with mode 1 builds equals the plane a context with mode 0 builds from the rule's output, for every level-0 kernel,
adopted frames, batches, parameter changes, refusals and the selection on the raw frame."""
import ctypes as C
import os

import numpy as np
import pytest

import equalize_expected as ee
from conftest import GOLDEN, read_pgm
from helpers import make_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, first_difference

pytestmark = pytest.mark.gpu
OPT_L0_LAZY_GRAD, OPT_L0_LEAN_FORM, OPT_FAIL_ALLOC_AFTER = 22, 23, 19
ERR_ARG, ERR_STATE, ERR_NOMEM = "error -1:", "error -3:", "error -4:"
LEVELS, SS = 2, 4


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """the context with mode 0 that builds from the rule's output"""
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


def _equalize(ctx, frame, tx, ty, clip_q8, pitch=None):
    ctx.set_equalize_params(mode=0, tiles_x=tx, tiles_y=ty, clip_q8=clip_q8)      # (klt_equalize_u8 does not look at the mode)
    nrows, ncols = frame.shape
    if pitch is None or pitch == ncols:
        return ctx.equalize(frame)
    wide = np.full((nrows, pitch), 0xA5, np.uint8)           # the padding holds bytes that must not count
    wide[:, :ncols] = frame
    return ctx.equalize(wide, ncols=ncols)


# ------------------------------------------------------------------------------------------------- (a) the kernel pair by name
# (ncols, nrows, pitch, tiles_x, tiles_y, clip_q8)
SHAPES = [(64, 48, 64, 8, 8, 768), (67, 45, 80, 3, 2, 768), (33, 17, 33, 4, 3, 1), (5, 3, 5, 5, 3, 768), (4, 4, 4, 1, 1, 0),
          (130, 70, 130, 64, 64, 768)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_p%d_%dx%d_%d" % s)
def test_kernel_pair_equals_the_rule(ctx, shape):
    ncols, nrows, pitch, tx, ty, clip_q8 = shape
    for name, frame in (("random", ee.random_frame(ncols, nrows, 3)), ("constant", ee.constant_frame(ncols, nrows)),
                        ("two bins", ee.two_bin_frame(ncols, nrows)), ("noise", np.random.RandomState(9).randint(0, 256, (nrows, ncols)).astype(np.uint8))):
        _same_bytes(_equalize(ctx, frame, tx, ty, clip_q8, pitch), ee.clahe(frame, tx, ty, clip_q8), "%s frame" % name)


@pytest.mark.parametrize("clip", [3.0, 40.0])
def test_kernel_pair_on_the_golden_frame(ctx, img0, clip):
    q8 = ee.clip_q8_of(clip)
    for frame in (img0, ee.darken_left_half(img0), ee.constant_frame(320, 240), ee.two_bin_frame(320, 240)):
        _same_bytes(_equalize(ctx, frame, 8, 8, q8), ee.clahe(frame, 8, 8, q8), "320 x 240, clip %g" % clip)


def test_kernel_pair_refuses_a_frame_smaller_than_the_grid(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError
    with pytest.raises(KltBackendError, match=ERR_ARG):
        _equalize(ctx, ee.random_frame(20, 10, 1), 64, 64, 768)
    _same_bytes(_equalize(ctx, ee.random_frame(20, 10, 1), 4, 2, 768), ee.clahe(ee.random_frame(20, 10, 1), 4, 2, 768), "the context after the refusal")


def test_kernel_pair_seeded_draws(ctx):
    for seed in range(40):
        frame, tx, ty, clip_q8, pitch = ee.trial(seed)
        _same_bytes(_equalize(ctx, frame, tx, ty, clip_q8, pitch), ee.clahe(frame, tx, ty, clip_q8),
                    "draw %d: %d x %d, pitch %d, %d x %d tiles, clip_q8 %d" % (seed, frame.shape[1], frame.shape[0], pitch, tx, ty, clip_q8))


def test_parameter_ranges(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError
    for bad in (dict(mode=2), dict(mode=-1), dict(tiles_x=0), dict(tiles_y=65), dict(clip_q8=-1), dict(clip_q8=(1 << 20) + 1)):
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.set_equalize_params(**bad)
    ctx.set_equalize_params(mode=0, tiles_x=64, tiles_y=1, clip_q8=1 << 20)
    ctx.set_equalize_params()


# ------------------------------------------------------------------------------------------------------ (b) through a slot
def _two_frames(ncols, nrows, seed):
    yy, xx = np.mgrid[0:nrows, 0:ncols]
    rs = np.random.RandomState(seed)
    out = []
    for k in range(2):
        f = 60 + 30 * np.sin(xx / (7.0 + k)) * np.cos(yy / (11.0 + k)) + rs.normal(0, 6, (nrows, ncols))
        f[:, : ncols // 2] = f[:, : ncols // 2] * 0.2 + 5          # a dark half
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def _planes(c, slot, levels=LEVELS):
    return [c.download_level(slot, p, l) for l in range(levels) for p in range(3)]


def _same_planes(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        bad = first_difference(a, b)
        assert not bad, "%s: plane %d of level %d: %s" % (what, i % 3, i // 3, bad)


# name -> (options, (ncols, nrows), frames, klt_level0_path code).  The sizes are those tests/test_gpu_l0_stream.py and
# tests/test_gpu_l0_lean.py reach each kernel with: 16 frames of 640 x 480 stay below the streaming kernels' grid bound, 32 frames of
# 256 x 2560 / 256 x 4096 are the smallest launches of the 64- and the 128-column geometry
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
    raw = _two_frames(ncols, nrows, ncols + nrows)
    want = [ee.clahe(f, 8, 8, 768) for f in raw]
    tc = make_tc(levels=LEVELS, ss=SS)
    look = sorted({0, 1, count - 1})
    try:
        for c, frames, mode in ((ctx, raw, 1), (plain, want, 0)):
            c.configure(tc)
            c.set_equalize_params(mode=mode)
            for opt, value in options.items():
                c.set_option(opt, value)
            for k in range(count):
                c.upload(k, frames[k % 2])
            c.build_pyramids_batch(list(range(count)), sync=True)
            assert c.level0_path()[0] == code, "%s: klt_level0_path says %d, the case was written for %d" % (path, c.level0_path()[0], code)
            assert c.level0_lean() == (options.get(OPT_L0_LAZY_GRAD) == 2)
            assert c.equalize_path() == mode
        for k in look:
            _same_bytes(ctx.download_equalized(k, ncols, nrows), want[k % 2], "%s: klt_download_equalized_u8 of slot %d" % (path, k))
            _same_planes(_planes(ctx, k), _planes(plain, k), "%s, slot %d" % (path, k))
        from pyfeaturetrack_amd._abi import KltBackendError
        with pytest.raises(KltBackendError, match=ERR_STATE):
            plain.download_equalized(0, ncols, nrows)
        # the slots' equalised frames are still valid: a rebuild enqueues no equalisation launch and gives the same planes
        ctx.build_pyramids_batch(list(range(count)), sync=True)
        assert ctx.equalize_path() == 0
        _same_planes(_planes(ctx, look[-1]), _planes(plain, look[-1]), "%s, rebuilt slot %d" % (path, look[-1]))
    finally:
        for c in (ctx, plain):
            for opt, value in DEFAULTS.items():
                c.set_option(opt, value)
            c.set_equalize_params()
            for k in range(2, count):
                c.slot_free(k)


# --------------------------------------------------------------------------------------------------------- (c) an adopted frame
def test_adopted_frame_is_read_and_never_written(ctx, plain, img0):
    img1 = read_pgm(os.path.join(GOLDEN, "img1.pgm"))
    raw = [ee.darken_left_half(img0), ee.darken_left_half(img1)]
    want = [ee.clahe(f, 8, 8, 768) for f in raw]
    tc = make_tc()
    both = np.concatenate([raw[0].ravel(), raw[1].ravel()])
    dev = ctx.device_alloc(both.nbytes + 64)
    try:
        ctx.device_write(dev, np.concatenate([both, np.full(64, 0x5A, np.uint8)]))
        ctx.configure(tc)
        ctx.set_equalize_params(mode=1)
        plain.configure(tc)
        for k in range(2):
            ctx.adopt_u8(k, dev + k * raw[0].size, 320, 240)
            plain.upload(k, want[k])
        ctx.build_pyramids_batch([0, 1], sync=True)
        plain.build_pyramids_batch([0, 1], sync=True)
        assert ctx.equalize_path() == 1
        for k in range(2):
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
        ctx.set_equalize_params()
        for k in range(2):
            ctx.slot_free(k)
        ctx.device_free(dev)


# ----------------------------------------------------------------------------------------------------------------- (d) a batch
def test_batch_of_two_sizes(ctx, plain):
    """four slots of two sizes in one klt_build_pyramids_batch_async: the frames of a size share the two launches"""
    tc = make_tc(levels=LEVELS, ss=SS)
    raw = _two_frames(203, 165, 1) + _two_frames(180, 200, 2)
    raw = [raw[0], raw[2], raw[1], raw[3]]                     # the sizes interleaved
    want = [ee.clahe(f, 8, 8, 768) for f in raw]
    try:
        ctx.configure(tc)
        ctx.set_equalize_params(mode=1)
        plain.configure(tc)
        for k in range(4):
            ctx.upload(k, raw[k])
            plain.upload(k, want[k])
        ctx.timing_enable(True)
        ctx.build_pyramids_batch([0, 1, 2, 3], sync=True)
        times = {t["name"]: t["launches"] for t in ctx.timing_read()}
        ctx.timing_enable(False)
        assert times.get("equalize_lut") == 2 and times.get("equalize_apply") == 2, times      # one pair of launches per size
        plain.build_pyramids_batch([0, 1, 2, 3], sync=True)
        assert ctx.equalize_path() == 1 and plain.equalize_path() == 0
        for k in range(4):
            _same_bytes(ctx.download_equalized(k, raw[k].shape[1], raw[k].shape[0]), want[k], "slot %d" % k)
            _same_planes(_planes(ctx, k), _planes(plain, k), "slot %d" % k)
        # one new frame: only its slot is equalised again; swapped slots take their equalised frames along
        ctx.upload(1, raw[3])
        ctx.swap_slots(0, 2)
        ctx.build_pyramids_batch([0, 1, 2, 3], sync=True)
        assert ctx.equalize_path() == 1
        for k, src in enumerate((2, 3, 0, 3)):
            _same_bytes(ctx.download_equalized(k, raw[src].shape[1], raw[src].shape[0]), want[src], "slot %d after the swap" % k)
            _same_planes(_planes(ctx, k), _planes(plain, src), "slot %d after the swap" % k)
    finally:
        ctx.timing_enable(False)
        ctx.set_equalize_params()
        for c in (ctx, plain):
            for k in range(4):
                c.slot_free(k)


# ------------------------------------------------------------------------------------------------------- (e) parameter changes
def test_parameter_changes_rebuild_from_the_new_parameters(ctx, plain, img0):
    tc = make_tc()
    dark = ee.darken_left_half(img0)
    levels = tc.nPyramidLevels
    try:
        ctx.configure(tc)
        plain.configure(tc)
        ctx.upload(0, dark)
        for mode, tx, ty, clip_q8 in ((1, 8, 8, 768), (1, 3, 5, 10240), (1, 3, 5, 0), (0, 3, 5, 0), (1, 8, 8, 768)):
            ctx.set_equalize_params(mode=mode, tiles_x=tx, tiles_y=ty, clip_q8=clip_q8)
            ctx.build_pyramids(0, sync=True)
            want = ee.clahe(dark, tx, ty, clip_q8) if mode else dark
            plain.upload(0, want)
            plain.build_pyramids(0, sync=True)
            assert ctx.equalize_path() == mode
            _same_planes(_planes(ctx, 0, levels), _planes(plain, 0, levels), "mode %d, %d x %d tiles, clip_q8 %d" % (mode, tx, ty, clip_q8))
            if mode:
                _same_bytes(ctx.download_equalized(0, 320, 240), want, "%d x %d tiles, clip_q8 %d" % (tx, ty, clip_q8))
    finally:
        ctx.set_equalize_params()
        ctx.slot_free(0)
        plain.slot_free(0)


# ---------------------------------------------------------------------------------------------------------------- (f) refusals
def test_refusals_leave_the_slot_usable(ctx, plain, img0):
    from pyfeaturetrack_amd._abi import KltBackendError, KltOutOfMemory
    tc = make_tc()
    levels = tc.nPyramidLevels
    small = ee.random_frame(40, 30, 2)
    try:
        ctx.configure(tc)
        plain.configure(tc)
        # an f32 slot
        ctx.set_equalize_params(mode=1)
        ctx.upload(0, img0.astype(np.float32))
        with pytest.raises(KltBackendError, match="error -3: equalisation takes 8-bit frames"):
            ctx.build_pyramids(0, sync=True)
        with pytest.raises(KltBackendError, match="error -3: equalisation takes 8-bit frames"):
            ctx.select(0, 10, use_pyramid=False)
        ctx.set_equalize_params(mode=0)
        ctx.build_pyramids(0, sync=True)
        plain.upload(0, img0.astype(np.float32))
        plain.build_pyramids(0, sync=True)
        _same_planes(_planes(ctx, 0, levels), _planes(plain, 0, levels), "the f32 slot with mode 0")
        # a frame smaller than the tile grid; an f32 slot beside an 8-bit one in a batch: nothing of the batch is built
        ctx.set_equalize_params(mode=1, tiles_x=64, tiles_y=64)
        ctx.upload(1, small)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.build_pyramids(1, sync=True)
        ctx.set_equalize_params(mode=1, tiles_x=4, tiles_y=3)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.build_pyramids_batch([1, 0], sync=True)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.download_equalized(1, 40, 30)
        # the allocation of the slot's equalised frame fails: KLT_ERR_NOMEM, and the next build has it
        one = make_tc(levels=1, ss=2)
        ctx.configure(one)
        plain.configure(one)
        ctx.set_equalize_params(mode=1, tiles_x=4, tiles_y=3)
        ctx.upload(1, small)
        ctx.build_pyramids(1, sync=True)                           # (everything else the build allocates is there now)
        ctx.slot_free(2)
        ctx.upload(2, small)
        ctx.set_equalize_params(mode=0)
        ctx.build_pyramids(2, sync=True)
        ctx.set_equalize_params(mode=1, tiles_x=4, tiles_y=3)
        ctx.set_option(OPT_FAIL_ALLOC_AFTER, 0)
        try:
            with pytest.raises(KltOutOfMemory):
                ctx.build_pyramids(2, sync=True)
        finally:
            ctx.set_option(OPT_FAIL_ALLOC_AFTER, -1)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.download_equalized(2, 40, 30)
        ctx.build_pyramids(2, sync=True)
        _same_bytes(ctx.download_equalized(2, 40, 30), ee.clahe(small, 4, 3, 768), "the slot after the failed allocation")
        plain.upload(2, ee.clahe(small, 4, 3, 768))
        plain.build_pyramids(2, sync=True)
        _same_planes(_planes(ctx, 2, 1), _planes(plain, 2, 1), "the slot after the failed allocation")
        ctx.set_equalize_params(mode=0)
        ctx.build_pyramids(2, sync=True)
        plain.upload(2, small)
        plain.build_pyramids(2, sync=True)
        _same_planes(_planes(ctx, 2, 1), _planes(plain, 2, 1), "that slot with mode 0")
    finally:
        ctx.set_option(OPT_FAIL_ALLOC_AFTER, -1)
        ctx.set_equalize_params()
        for c in (ctx, plain):
            for k in range(3):
                c.slot_free(k)


# ------------------------------------------------------------------------------------------------------ (g) raw-frame selection
@pytest.mark.parametrize("smooth", [True, False], ids=["smoothed", "unsmoothed"])
def test_selection_on_the_raw_frame(ctx, plain, img0, smooth):
    tc = make_tc(smoothBeforeSelecting=smooth)
    dark = ee.darken_left_half(img0)
    want = ee.clahe(dark, 8, 8, 768)
    try:
        ctx.configure(tc)
        ctx.set_equalize_params(mode=1)
        plain.configure(tc)
        ctx.upload(0, dark)                                        # a fresh upload: the selection finds the equalised frame stale
        plain.upload(0, want)
        got, placed = ctx.select(0, 300, use_pyramid=False)
        exp, placed_exp = plain.select(0, 300, use_pyramid=False)
        assert placed == placed_exp and got.tobytes() == exp.tobytes()
        _same_bytes(ctx.download_equalized(0, 320, 240), want, "the frame the selection read")
        if smooth:
            # what the stage is for (the default selection; tests/test_equalize_rule.py has the oracle's figures): more features in the dark half
            ctx.set_equalize_params(mode=0)
            darksel, _ = ctx.select(0, 300, use_pyramid=False)
            assert int(((got["val"] >= 0) & (got["x"] < 160)).sum()) > int(((darksel["val"] >= 0) & (darksel["x"] < 160)).sum())
    finally:
        ctx.set_equalize_params()
        ctx.slot_free(0)
        plain.slot_free(0)
