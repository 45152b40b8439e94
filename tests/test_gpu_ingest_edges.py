"""The two ingest stages on the device at the bounds of their loops and of their 32-bit arithmetic (tables, class functions and draws:
tests/ingest_edges_expected.py; what each entry reaches: tests/test_ingest_edges_rule.py), byte for byte against the numpy rules: the
kernels by name (klt_equalize_u8, klt_remap_u8) on every table entry and on seeded draws, the two refused shapes beside the largest
accepted one, and through slots -- more than KLT_MAX_BATCH slots in one build, every slot another frame, every slot downloaded; adopted
frames that start at every residue of 16."""
import ctypes as C
import time

import numpy as np
import pytest

import equalize_expected as ee
import ingest_edges_expected as ie
import remap_expected as re_
from helpers import make_tc
from pyramid_expected import expected_path, first_difference

pytestmark = pytest.mark.gpu
OPT_L0_LAZY_GRAD = 22
LEVELS, SS = 2, 4
NC, NR = 67, 45                                              # the slots' frames


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """the context with both stages off that builds from the rules' output"""
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if bad.size:
        y, x = divmod(int(bad[0]), got.shape[1])
        raise AssertionError("%s: %d of %d bytes differ; first at (x %d, y %d): %d, the rule says %d" %
                             (what, bad.size, got.size, x, y, got[y, x], want[y, x]))


def _padded(frame, pitch):
    nrows, ncols = frame.shape
    if pitch == ncols:
        return frame
    wide = np.full((nrows, pitch), 0xA5, np.uint8)           # the padding holds bytes that must not count
    wide[:, :ncols] = frame
    return wide


def _equalize(ctx, frame, tx, ty, clip_q8, pitch=None):
    ctx.set_equalize_params(mode=0, tiles_x=tx, tiles_y=ty, clip_q8=clip_q8)      # (klt_equalize_u8 does not look at the mode)
    return ctx.equalize(_padded(frame, pitch or frame.shape[1]), ncols=frame.shape[1])


# ----------------------------------------------------------------------------------------------------------- the kernels by name
@pytest.mark.parametrize("name", list(ie.CLAHE_EDGES))
def test_clahe_edge(ctx, name):
    case = ie.CLAHE_EDGES[name]
    want, _, seconds = ie.clahe_reference(name)
    t0 = time.time()
    got = _equalize(ctx, ie.clahe_frame(case), case.tiles_x, case.tiles_y, case.clip_q8, case.pitch)
    print("%s: the rule %.2f s, klt_equalize_u8 %.3f s" % (name, seconds, time.time() - t0))
    _same_bytes(got, want, name)


def test_clahe_refuses_the_shapes_past_the_bound(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError
    for ncols, nrows, tx, ty in ie.CLAHE_REFUSED:
        with pytest.raises(KltBackendError, match="error -1: equalisation: tiles too large"):
            _equalize(ctx, np.zeros((nrows, ncols), np.uint8), tx, ty, 768)
    name = "large_a_4096x4112_2x2"
    case = ie.CLAHE_EDGES[name]
    _same_bytes(_equalize(ctx, ie.clahe_frame(case), case.tiles_x, case.tiles_y, case.clip_q8), ie.clahe_reference(name)[0], "the context after the refusals")


@pytest.mark.parametrize("name", list(ie.REMAP_EDGES))
def test_remap_edge(ctx, name):
    case = ie.REMAP_EDGES[name]
    frame, (mx, my), want, _ = ie.remap_reference(name)
    try:
        ctx.set_remap(mx, my)
        _same_bytes(ctx.remap(_padded(frame, case.pitch), ncols=case.ncols), want, name)
    finally:
        ctx.set_remap()


@pytest.mark.parametrize("seed", ie.DRAW_SEEDS)
def test_clahe_draw(ctx, seed):
    frame, tx, ty, clip_q8, pitch = ie.clahe_draw(seed)
    _same_bytes(_equalize(ctx, frame, tx, ty, clip_q8, pitch), ee.clahe(frame, tx, ty, clip_q8),
                "draw %d: %d x %d, pitch %d, %d x %d tiles, clip_q8 %d" % (seed, frame.shape[1], frame.shape[0], pitch, tx, ty, clip_q8))


@pytest.mark.parametrize("seed", ie.DRAW_SEEDS)
def test_remap_draw(ctx, seed):
    frame, (mx, my), pitch, name = ie.remap_draw(seed)
    try:
        ctx.set_remap(mx, my)
        _same_bytes(ctx.remap(_padded(frame, pitch), ncols=frame.shape[1]), re_.remap(frame, mx, my),
                    "draw %d: %d x %d, pitch %d, %s map" % (seed, frame.shape[1], frame.shape[0], pitch, name))
    finally:
        ctx.set_remap()


# ------------------------------------------------------------------------------------------------------------- through a slot
def _planes(c, slot):
    return [c.download_level(slot, p, l) for l in range(LEVELS) for p in range(3)]


def _same_planes(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        bad = first_difference(a, b)
        assert not bad, "%s: plane %d of level %d: %s" % (what, i % 3, i // 3, bad)


def _launches(c, slots):
    """one synchronous build of `slots` -> the launches of every timed family"""
    c.timing_enable(True)
    try:
        c.build_pyramids_batch(list(slots), sync=True)
        return {t["name"]: t["launches"] for t in c.timing_read()}
    finally:
        c.timing_enable(False)


def _clean(contexts, count):
    for c in contexts:
        c.timing_enable(False)
        c.set_option(OPT_L0_LAZY_GRAD, 1)
        c.set_remap()
        c.set_equalize_params()
        for k in range(count):
            c.slot_free(k)


def _plain_planes(plain, frames):
    """the planes a context without the stages builds from `frames` (one batch, slots 0 ..)"""
    for k, f in enumerate(frames):
        plain.upload(k, f)
    plain.build_pyramids_batch(list(range(len(frames))), sync=True)
    return [_planes(plain, k) for k in range(len(frames))]


MAP = ("rotation", 9.0)


def _slot_map():
    return re_.rotation_map(NC, NR, MAP[1])


def _remap_33(ctx, plain):
    n = ie.MAX_BATCH + 1
    raw = [ie.slot_frame(NC, NR, k) for k in range(n)]
    mx, my = _slot_map()
    want = [re_.remap(f, mx, my) for f in raw]
    ctx.set_remap(mx, my)
    for k in range(n):
        ctx.upload(k, raw[k])
    times = _launches(ctx, range(n))
    assert times.get("remap") == 2 and ctx.remap_path() == 1, times      # 32 frames and 1
    for k in range(n):
        _same_bytes(ctx.download_remapped(k, NC, NR), want[k], "klt_download_remapped_u8 of slot %d" % k)
    look = (0, ie.MAX_BATCH - 1, ie.MAX_BATCH)
    for k, planes in zip(look, _plain_planes(plain, [want[k] for k in look])):
        _same_planes(_planes(ctx, k), planes, "slot %d" % k)


def _clahe_36(ctx, plain, clip_q8):
    """33 slots of 67 x 45 with 3 slots of 40 x 30 between them: launches of 32 frames, of 3 and of the one left over"""
    small_at = (5, 17, 30)
    n = ie.MAX_BATCH + 1 + len(small_at)
    raw = [ie.slot_frame(40, 30, k) if k in small_at else ie.slot_frame(NC, NR, k) for k in range(n)]
    want = [ee.clahe(f, 3, 2, clip_q8) for f in raw]
    ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=clip_q8)
    for k in range(n):
        ctx.upload(k, raw[k])
    times = _launches(ctx, range(n))
    assert times.get("equalize_lut") == 3 and times.get("equalize_apply") == 3 and ctx.equalize_path() == 1, times
    for k in range(n):
        _same_bytes(ctx.download_equalized(k, raw[k].shape[1], raw[k].shape[0]), want[k], "klt_download_equalized_u8 of slot %d" % k)
    look = (0, small_at[0], n - 1)
    for k in look:
        planes = _plain_planes(plain, [want[k]])[0]
        _same_planes(_planes(ctx, k), planes, "slot %d" % k)


def _both_33(ctx, plain):
    n = ie.MAX_BATCH + 1
    raw = [ie.slot_frame(NC, NR, 40 + k) for k in range(n)]
    mx, my = _slot_map()
    remapped = [re_.remap(f, mx, my) for f in raw]
    want = [ee.clahe(f, 3, 2, 768) for f in remapped]
    ctx.set_remap(mx, my)
    ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
    for k in range(n):
        ctx.upload(k, raw[k])
    times = _launches(ctx, range(n))
    assert times.get("remap") == 2 and times.get("equalize_lut") == 2 and times.get("equalize_apply") == 2, times
    for k in range(n):
        _same_bytes(ctx.download_remapped(k, NC, NR), remapped[k], "klt_download_remapped_u8 of slot %d" % k)
        _same_bytes(ctx.download_equalized(k, NC, NR), want[k], "klt_download_equalized_u8 of slot %d" % k)
    look = (0, ie.MAX_BATCH - 1, ie.MAX_BATCH)
    for k, planes in zip(look, _plain_planes(plain, [want[k] for k in look])):
        _same_planes(_planes(ctx, k), planes, "slot %d" % k)


def _batch_32(ctx, plain, lazy, stage):
    """one launch of KLT_MAX_BATCH distinct frames: the level-0 kernel that size takes reads slot b's own copy"""
    n = ie.MAX_BATCH
    raw = [ie.slot_frame(NC, NR, 80 + k) for k in range(n)]
    mx, my = _slot_map()
    if stage == "remap":
        want = [re_.remap(f, mx, my) for f in raw]
        ctx.set_remap(mx, my)
    else:
        want = [ee.clahe(f, 3, 2, 768) for f in raw]
        ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
    for c in (ctx, plain):
        c.set_option(OPT_L0_LAZY_GRAD, lazy)
    for k in range(n):
        ctx.upload(k, raw[k])
    ctx.build_pyramids_batch(list(range(n)), sync=True)
    planes = _plain_planes(plain, want)
    # the kernel a context without the stages takes for this launch, which is what pyramid_expected says of the size
    tc = make_tc(levels=LEVELS, ss=SS)
    assert ctx.level0_path() == plain.level0_path() == expected_path(NC, NR, n, False, LEVELS, SS, tc.smooth_sigma_fact)
    assert ctx.level0_lean() == plain.level0_lean()
    for k in range(n):
        got = ctx.download_remapped(k, NC, NR) if stage == "remap" else ctx.download_equalized(k, NC, NR)
        _same_bytes(got, want[k], "slot %d" % k)
        _same_planes(_planes(ctx, k), planes[k], "slot %d" % k)


def _adopted_16(ctx, plain, stages):
    """16 frames back to back in one device buffer: 67 * 45 = 3015 = 16 * 188 + 7 bytes each, so they start at every residue of 16"""
    n, size = 16, NC * NR
    raw = [ie.slot_frame(NC, NR, 120 + k) for k in range(n)]
    mx, my = _slot_map()
    want_rm = [re_.remap(f, mx, my) for f in raw] if "remap" in stages else raw
    want = [ee.clahe(f, 3, 2, 768) for f in want_rm] if "clahe" in stages else want_rm
    guard = np.full(64, 0x5A, np.uint8)
    buf = np.concatenate([f.ravel() for f in raw] + [guard])
    dev = ctx.device_alloc(buf.nbytes)
    try:
        assert dev % 16 == 0 and sorted((dev + k * size) % 16 for k in range(n)) == list(range(16))
        ctx.device_write(dev, buf)
        if "remap" in stages:
            ctx.set_remap(mx, my)
        if "clahe" in stages:
            ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
        for k in range(n):
            ctx.adopt_u8(k, dev + k * size, NC, NR)
        ctx.build_pyramids_batch(list(range(n)), sync=True)
        assert ctx.remap_path() == ("remap" in stages) and ctx.equalize_path() == ("clahe" in stages)
        for k in range(n):
            if "remap" in stages:
                _same_bytes(ctx.download_remapped(k, NC, NR), want_rm[k], "klt_download_remapped_u8 of slot %d (residue %d)" % (k, (k * size) % 16))
            if "clahe" in stages:
                _same_bytes(ctx.download_equalized(k, NC, NR), want[k], "klt_download_equalized_u8 of slot %d (residue %d)" % (k, (k * size) % 16))
        look = (1, 8, 15)
        for k, planes in zip(look, _plain_planes(plain, [want[k] for k in look])):
            _same_planes(_planes(ctx, k), planes, "adopted slot %d" % k)
        # the caller's buffer, and the guard bytes behind it, as they were
        ctx.sync()
        back = np.zeros(buf.nbytes, np.uint8)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(back.ctypes.data, dev, back.nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert np.array_equal(back, buf)
    finally:
        _clean((ctx,), n)
        ctx.device_free(dev)


# ---- a call that the SECOND stage refuses enqueues nothing and leaves the slots' copies as they were (ensure_ingested: every refusal of
# every stage in front of the first allocation and the first launch)
SMALL = (40, 30)
STAGE_FAMILIES = ("remap", "equalize_lut", "equalize_apply")
GRID_REFUSAL = "error -1: equalisation: the frame is smaller than the tile grid"
NO_REMAPPED, NO_EQUALISED = "error -3: the slot holds no remapped frame", "error -3: the slot holds no equalised frame"


def _grid_past_the_frame(ctx, count):
    """a map for 40 x 30 and a tile grid 64 wide, which 40 columns do not fit; `count` slots uploaded -> (the frames remapped, then
    equalised under 3 x 2 tiles)"""
    raw = [ie.slot_frame(SMALL[0], SMALL[1], 160 + k) for k in range(count)]
    mx, my = re_.rotation_map(SMALL[0], SMALL[1], MAP[1])
    remapped = [re_.remap(f, mx, my) for f in raw]
    ctx.set_remap(mx, my)
    ctx.set_equalize_params(mode=1, tiles_x=64, tiles_y=2, clip_q8=768)
    for k in range(count):
        ctx.upload(k, raw[k])
    return remapped, [ee.clahe(f, 3, 2, 768) for f in remapped]


def _refused(ctx, call, message, slots):
    """`call` raises with `message`, no stage family shows a launch, and no slot holds a copy afterwards"""
    from pyfeaturetrack_amd._abi import KltBackendError
    ctx.timing_enable(True)
    try:
        with pytest.raises(KltBackendError, match=message):
            call()
        times = {t["name"]: t["launches"] for t in ctx.timing_read()}
    finally:
        ctx.timing_enable(False)
    assert not any(times.get(f) for f in STAGE_FAMILIES), times
    for k in slots:
        with pytest.raises(KltBackendError, match=NO_REMAPPED):
            ctx.download_remapped(k, *SMALL)
        with pytest.raises(KltBackendError, match=NO_EQUALISED):
            ctx.download_equalized(k, *SMALL)


def _refused_build(ctx, plain):
    remapped, want = _grid_past_the_frame(ctx, 2)
    _refused(ctx, lambda: ctx.build_pyramids_batch([0, 1], sync=True), GRID_REFUSAL, (0, 1))
    # a frame of another size beside them: the first stage's refusal, and nothing enqueued for slot 0 either
    ctx.upload(2, ie.slot_frame(NC, NR, 162))
    _refused(ctx, lambda: ctx.build_pyramids_batch([0, 2], sync=True), "error -1: remapping: the frame is 67 by 45, the map 40 by 30", (0, 1))
    ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
    times = _launches(ctx, (0, 1))
    assert [times.get(f) for f in STAGE_FAMILIES] == [1, 1, 1] and ctx.remap_path() == 1 and ctx.equalize_path() == 1, times
    for k, planes in zip((0, 1), _plain_planes(plain, want)):
        _same_bytes(ctx.download_remapped(k, *SMALL), remapped[k], "klt_download_remapped_u8 of slot %d" % k)
        _same_bytes(ctx.download_equalized(k, *SMALL), want[k], "klt_download_equalized_u8 of slot %d" % k)
        _same_planes(_planes(ctx, k), planes, "slot %d" % k)


def _refused_selection(ctx, plain):
    tc = make_tc(levels=1, ss=2, window=3)                   # (the default border leaves no candidate in a frame this small)
    ctx.configure(tc)
    plain.configure(tc)
    remapped, want = _grid_past_the_frame(ctx, 1)
    _refused(ctx, lambda: ctx.select(0, 40, use_pyramid=False), GRID_REFUSAL, (0,))
    ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
    got, placed = ctx.select(0, 40, use_pyramid=False)
    plain.upload(0, want[0])
    exp, placed_exp = plain.select(0, 40, use_pyramid=False)
    assert placed == placed_exp and placed > 0 and got.tobytes() == exp.tobytes()
    _same_bytes(ctx.download_remapped(0, *SMALL), remapped[0], "the remapped frame the selection read")
    _same_bytes(ctx.download_equalized(0, *SMALL), want[0], "the equalised frame the selection read")


SLOT_CASES = {
    "remap_33_slots": lambda c, p: _remap_33(c, p),
    "clahe_33_and_3_slots_clip_768": lambda c, p: _clahe_36(c, p, 768),
    "clahe_33_and_3_slots_clip_2_20": lambda c, p: _clahe_36(c, p, 1 << 20),
    "remap_then_clahe_33_slots": lambda c, p: _both_33(c, p),
    "batch_32_lazy_grad_2_clahe": lambda c, p: _batch_32(c, p, 2, "clahe"),
    "batch_32_lazy_grad_2_remap": lambda c, p: _batch_32(c, p, 2, "remap"),
    "batch_32_lazy_grad_0_clahe": lambda c, p: _batch_32(c, p, 0, "clahe"),
    "batch_32_lazy_grad_0_remap": lambda c, p: _batch_32(c, p, 0, "remap"),
    "adopted_16_residues_clahe": lambda c, p: _adopted_16(c, p, ("clahe",)),
    "adopted_16_residues_remap": lambda c, p: _adopted_16(c, p, ("remap",)),
    "adopted_16_residues_remap_then_clahe": lambda c, p: _adopted_16(c, p, ("remap", "clahe")),
    "second_stage_refusal_enqueues_nothing": lambda c, p: _refused_build(c, p),
    "second_stage_refusal_enqueues_nothing_selection": lambda c, p: _refused_selection(c, p),
}


@pytest.mark.parametrize("case", list(SLOT_CASES))
def test_slot_case(ctx, plain, case):
    tc = make_tc(levels=LEVELS, ss=SS)
    try:
        ctx.configure(tc)
        plain.configure(tc)
        SLOT_CASES[case](ctx, plain)
    finally:
        _clean((ctx, plain), ie.MAX_BATCH + 4)
