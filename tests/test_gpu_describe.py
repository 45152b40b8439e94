"""The describe launch on the device (include/klt_gpu.h, "descriptors", rule 1) against the rule in numpy
(tests/describe_expected.py), byte for byte, in both modes: frames from 1 x 1 up, features on every edge and at the half-pixel
positions where the centre changes, the wavefront and workgroup edges of the list, seeded draws; through a slot behind the ingest
stages, an adopted frame, a swap and an asynchronous upload; every refusal and a failed allocation."""
import ctypes as C
import os

import numpy as np
import pytest

import describe_expected as de
from conftest import GOLDEN, read_pgm
from helpers import make_tc

pytestmark = pytest.mark.gpu
OPT_FAIL_ALLOC_AFTER = 19
ERR_ARG, ERR_STATE = "error -1:", "error -3:"
MODES = (de.UPRIGHT, de.STEERED)


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def img0():
    return read_pgm(os.path.join(GOLDEN, "img0.pgm"))


def _same_records(got, want, what):
    assert got.dtype == de.DESC_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, "%s: %d of %d records differ; first %d: %r, the rule says %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


def _describe(ctx, frame, feats, mode, slot=0, sync_entry=False):
    ctx.upload(slot, frame)
    ctx.set_descriptor_params(mode)
    return ctx.describe(slot, feats, sync_entry=sync_entry).view(de.DESC_DTYPE)


def edge_features(ncols, nrows):
    """the four corners, a point on each edge, the centre, half-pixel positions, the positions where a centre enters or leaves the frame,
    lost and non-finite records"""
    mx, my = (ncols - 1) / 2.0, (nrows - 1) / 2.0
    pts = [(0, 0), (ncols - 1, 0), (0, nrows - 1), (ncols - 1, nrows - 1), (mx, 0), (mx, nrows - 1), (0, my), (ncols - 1, my), (mx, my),
           (int(mx) + 0.5, int(my) + 0.5), (int(mx) + 0.5, my), (-0.5, 0), (-0.6, 0), (ncols - 0.5, 0), (ncols - 0.51, 0),
           (0, -0.5), (0, -0.6), (0, nrows - 0.5), (0, nrows - 0.51), (mx, my), (mx, my), (mx, my), (mx, my), (mx, my)]
    f = de.features([p[0] for p in pts], [p[1] for p in pts])
    f["val"][-5] = -1                                        # lost
    f["val"][-4] = 12345                                     # a freshly selected feature: val is its eigenvalue
    f["x"][-3] = np.nan
    f["y"][-2] = np.inf
    f["x"][-1] = -np.inf
    f["aux"] = np.arange(len(f))
    return f


FRAMES = [(1, 1), (5, 3), (31, 31), (37, 41), (64, 48)]


@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "%dx%d" % s)
def test_small_frames_equal_the_rule(ctx, shape):
    ncols, nrows = shape
    rng = np.random.default_rng(ncols * 100 + nrows)
    feats = edge_features(ncols, nrows)
    for kind in ("random", "two", "constant"):
        frame = de.random_frame(rng, ncols, nrows, kind)
        for mode in MODES:
            _same_records(_describe(ctx, frame, feats, mode), de.describe(frame, feats, mode), "%s frame, mode %d" % (kind, mode))


def test_pitch_wider_than_the_frame_through_the_host_call(ctx):
    """klt_upload_u8 with pitch > ncols, then klt_describe (the synchronous entry point over the library's staging buffers)"""
    rng = np.random.default_rng(5)
    frame = de.random_frame(rng, 64, 48, "random")
    wide = np.full((48, 80), 0xA5, np.uint8)                 # the padding holds bytes that must not count
    wide[:, :64] = frame
    ctx._check(ctx._lib.klt_upload_u8(ctx._h, 0, wide.ctypes.data, 64, 48, 80))
    feats = edge_features(64, 48)
    for mode in MODES:
        ctx.set_descriptor_params(mode)
        got = ctx.describe(0, feats, sync_entry=True).view(de.DESC_DTYPE)
        _same_records(got, de.describe(frame, feats, mode), "pitch 80, mode %d" % mode)


def test_golden_frame_and_list_lengths(ctx, img0):
    """320 x 240; n over the wavefront and workgroup edges (four features per workgroup), 0 included"""
    rng = np.random.default_rng(11)
    pool = np.concatenate([edge_features(320, 240), de.random_features(rng, 257, 320, 240)])
    want = {mode: de.describe(img0, pool, mode) for mode in MODES}
    ctx.upload(0, img0)
    for mode in MODES:
        ctx.set_descriptor_params(mode)
        for n in (0, 1, 3, 4, 5, 63, 64, 65, 257, len(pool)):
            for sync_entry in (False, True):
                got = ctx.describe(0, pool[:n], sync_entry=sync_entry).view(de.DESC_DTYPE)
                _same_records(got, want[mode][:n], "n %d, mode %d, sync_entry %s" % (n, mode, sync_entry))
        assert (want[mode]["val"] == 1).sum() > 150 and (want[mode]["val"] == 0).sum() > 10
    assert len(set(want[de.STEERED]["orientation"].tolist())) > 8           # the steered form takes many bins on this frame


def test_seeded_draws(ctx):
    for seed in range(40):
        frame, feats, mode = de.describe_draw(seed)
        _same_records(_describe(ctx, frame, feats, mode), de.describe(frame, feats, mode),
                      "draw %d: %d x %d, %d features, mode %d" % (seed, frame.shape[1], frame.shape[0], len(feats), mode))


# ------------------------------------------------------------------------------------------------------------- through a slot
def _shear_map(ncols, nrows):
    yy, xx = np.mgrid[0:nrows, 0:ncols]
    return ((xx * 256 + yy * 37 - 900).astype(np.int32), (yy * 256 - xx * 11 + 300).astype(np.int32))


@pytest.mark.parametrize("stages", ["remap", "clahe", "both"])
def test_behind_the_ingest_stages(ctx, img0, stages):
    """after a build with the stage(s) on, the descriptors are the rule's on the frame the slot's readers see; and without a build"""
    tc = make_tc()
    feats = np.concatenate([edge_features(320, 240), de.random_features(np.random.default_rng(3), 70, 320, 240)])
    try:
        ctx.configure(tc)
        if stages in ("remap", "both"):
            ctx.set_remap(*_shear_map(320, 240))
        if stages in ("clahe", "both"):
            ctx.set_equalize_params(mode=1)
        ctx.upload(0, img0)
        ctx.build_pyramids(0, sync=True)
        seen = ctx.download_equalized(0, 320, 240) if stages != "remap" else ctx.download_remapped(0, 320, 240)
        assert not np.array_equal(seen, img0)
        for mode in MODES:
            ctx.set_descriptor_params(mode)
            _same_records(ctx.describe(0, feats).view(de.DESC_DTYPE), de.describe(seen, feats, mode), "%s, built, mode %d" % (stages, mode))
        # a slot that was never built: the describe call runs the chain itself
        ctx.upload(1, img0)
        ctx.set_descriptor_params(de.UPRIGHT)
        _same_records(ctx.describe(1, feats).view(de.DESC_DTYPE), de.describe(seen, feats, de.UPRIGHT), "%s, not built" % stages)
    finally:
        ctx.set_remap()
        ctx.set_equalize_params()
        for k in range(2):
            ctx.slot_free(k)


def test_adopted_frame_swap_and_asynchronous_upload(ctx, img0):
    img1 = read_pgm(os.path.join(GOLDEN, "img1.pgm"))
    feats = np.concatenate([edge_features(320, 240), de.random_features(np.random.default_rng(4), 40, 320, 240)])
    want = [de.describe(f, feats, de.STEERED) for f in (img0, img1)]
    ctx.set_descriptor_params(de.STEERED)
    dev = ctx.device_alloc(img0.size + 64)
    try:
        # adopted: read in place and never written, the guard bytes behind it as they were
        ctx.device_write(dev, np.concatenate([img0.ravel(), np.full(64, 0x5A, np.uint8)]))
        ctx.adopt_u8(0, dev, 320, 240)
        _same_records(ctx.describe(0, feats).view(de.DESC_DTYPE), want[0], "adopted frame")
        back = np.zeros(img0.size + 64, np.uint8)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(back.ctypes.data, dev, back.nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert np.array_equal(back[:img0.size], img0.ravel()) and (back[img0.size:] == 0x5A).all()
        # swapped slots take their frames along
        ctx.upload(1, img1)
        ctx.swap_slots(0, 1)
        _same_records(ctx.describe(0, feats).view(de.DESC_DTYPE), want[1], "slot 0 after the swap")
        _same_records(ctx.describe(1, feats).view(de.DESC_DTYPE), want[0], "slot 1 after the swap")
        # an asynchronous upload immediately before: the launch waits for the copy on the device
        staged = ctx.pinned_array((240, 320))
        for k, frame in enumerate((img1, img0, img1)):
            staged[:] = frame
            ctx.upload_async(2, staged)
            _same_records(ctx.describe(2, feats).view(de.DESC_DTYPE), want[1 - k % 2], "asynchronous upload %d" % k)
            ctx.upload_wait()
    finally:
        for k in range(3):
            ctx.slot_free(k)
        ctx.device_free(dev)


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing_and_a_good_call_follows(ctx, img0):
    from pyfeaturetrack_amd._abi import KltBackendError
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    feats = edge_features(320, 240)
    want = de.describe(img0, feats, de.UPRIGHT)
    FB_IN, FB_DESC, FB_VIEW = 100, 101, 102
    try:
        ctx.set_descriptor_params(de.UPRIGHT)
        for bad_mode in (0, 3, -1):
            with pytest.raises(KltBackendError, match=ERR_ARG):
                ctx.set_descriptor_params(bad_mode)
        ctx.upload(0, img0)
        ctx.upload(1, img0.astype(np.float32))
        ctx.featbuf_upload(FB_IN, feats.astype(FEAT_DTYPE))
        ctx.featbuf_view(FB_VIEW, FB_IN, 0, len(feats))
        ctx.timing_enable(True)
        with pytest.raises(KltBackendError, match="error -3: slot has no frame"):
            ctx.describe_async(7000, FB_IN, FB_DESC, len(feats))                 # a slot never used
        ctx.slot_free(2)
        with pytest.raises(KltBackendError, match="error -3: slot has no frame"):
            ctx.describe_async(2, FB_IN, FB_DESC, len(feats))                    # a slot without a frame
        with pytest.raises(KltBackendError, match="error -3: descriptors take 8-bit frames"):
            ctx.describe_async(1, FB_IN, FB_DESC, len(feats))
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.describe_async(0, FB_IN, FB_IN, len(feats))                      # the same buffer by index
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.describe_async(0, FB_IN, FB_VIEW, len(feats))                    # ... and by address
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.describe_async(0, FB_IN, FB_DESC, -1)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.describe_async(0, FB_IN, -1, len(feats))
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.describe_async(0, FB_IN, FB_DESC, len(feats) + 1)                # the list is shorter
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.describe_async(0, 103, FB_DESC, 1)                               # no such list
        ctx.describe_async(0, FB_IN, FB_DESC, 0)                                 # n == 0: nothing to do
        ctx.sync()
        assert not [t for t in ctx.timing_read() if t["name"] == "describe"]
        assert ctx.featbuf_devptr(FB_DESC) is None                               # ... and nothing was allocated for the records
        ctx.describe_async(0, FB_IN, FB_DESC, len(feats))
        _same_records(ctx.descriptor_download(FB_DESC, len(feats)).view(de.DESC_DTYPE), want, "the good call after the refusals")
        assert [t["launches"] for t in ctx.timing_read() if t["name"] == "describe"] == [1]
    finally:
        ctx.timing_enable(False)
        for k in range(3):
            ctx.slot_free(k)


def test_failed_allocation_then_a_good_call(img0):
    """fresh contexts: a first describe call allocates the list's buffer, the pattern and the records; with the k-th of them refused the
    call is KLT_ERR_NOMEM, and the same call repeated is good"""
    from pyfeaturetrack_amd._abi import KltOutOfMemory
    from pyfeaturetrack_amd.backend import Context
    feats = edge_features(320, 240)
    want = de.describe(img0, feats, de.STEERED)
    failed = 0
    for k in range(8):
        c = Context(0)
        try:
            c.upload(0, img0)
            c.set_descriptor_params(de.STEERED)
            c.set_option(OPT_FAIL_ALLOC_AFTER, k)
            try:
                got = c.describe(0, feats)
            except KltOutOfMemory:
                got = None
                failed += 1
            finally:
                c.set_option(OPT_FAIL_ALLOC_AFTER, -1)
            if got is None:
                got = c.describe(0, feats)
                _same_records(got.view(de.DESC_DTYPE), want, "the call after failed allocation %d" % k)
            else:
                _same_records(got.view(de.DESC_DTYPE), want, "no allocation left to fail (%d)" % k)
                break
        finally:
            c.close()
    assert 3 <= failed < 8, failed
