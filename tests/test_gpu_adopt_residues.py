"""Adopted frames (klt_slot_adopt_u8) that start at any byte, read in place by every kernel that takes a caller's frame: the level-0
kernels of tests/adopt_expected.ADOPT_L0 (what the table covers and that the comparison would notice a wrong alignment rule:
tests/test_adopt_rule.py, no GPU), the selection on the raw frame, the describe launch, and a batch behind the CLAHE stage that is then
switched off.  One clip buffer per test, frames at residues k % 16 of a base on 16 bytes (every class of addr % 4 mixed in one launch),
0x5A in every gap and 64 guard bytes behind; everything is compared bit for bit with the same frames uploaded, frames 0 .. 3 (residues
0 .. 3) of the level-0 cases with the CPU oracle as well, and the caller's buffer is read back afterwards: read and never written."""
import ctypes as C

import numpy as np
import pytest

import adopt_expected as ae
import describe_expected as de
import equalize_expected as ee
import ingest_edges_expected as ie
from helpers import make_tc
from pyramid_expected import OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, expected_path, first_difference, tc_of
from test_gpu_describe import edge_features
from test_gpu_l0_lean_wave import KLT_OPT_L0_LEAN_FORM, OPT_L0_LAZY_GRAD, _header_default_form

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    """a second context that only ever sees uploaded frames"""
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


class Clip:
    """a layout of adopt_expected.pack in device memory of the context"""

    def __init__(self, ctx, frames, residues=None):
        self.ctx, self.lay = ctx, ae.pack(frames, residues)
        self.dev = ctx.device_alloc(self.lay.buf.nbytes)
        try:
            self.addr = ae.addresses(self.dev, self.lay)
            ctx.device_write(self.dev, self.lay.buf)
        except BaseException:
            ctx.device_free(self.dev)
            raise

    def adopt(self, shape, slots=None):
        nrows, ncols = shape
        for k, a in enumerate(self.addr):
            self.ctx.adopt_u8(k if slots is None else slots[k], a, ncols, nrows)

    def assert_untouched(self):
        """frames, gaps and guard bytes as they were written"""
        self.ctx.sync()
        back = np.zeros(self.lay.buf.nbytes, np.uint8)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(back.ctypes.data, self.dev, back.nbytes, 2) == 0          # hipMemcpyDeviceToHost
        bad = np.flatnonzero(back != self.lay.buf)
        assert not bad.size, "%d bytes of the caller's buffer changed; first at offset %d" % (bad.size, bad[0])

    def free(self):
        self.ctx.device_free(self.dev)


def _planes(c, slot, levels):
    return [[c.download_level(slot, p, l) for p in range(3)] for l in range(levels)]


def _same(what, got, want, k, l, p):
    bad = first_difference(got, want)
    assert not bad, "%s: frame %d, plane %d of level %d: %s" % (what, k, p, l, bad)


# ------------------------------------------------------------------------------------------------------------------- level-0 kernels
def _options(ctx, a, lazy, form):
    ctx.set_option(OPT_FUSED_KERNELS, a.case.fused)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, a.stream)
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)
    ctx.set_option(KLT_OPT_L0_LEAN_FORM, form)


def _restore(ctx):
    ctx.set_option(OPT_FUSED_KERNELS, 1)                 # (the defaults)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, 2)
    ctx.set_option(OPT_L0_LAZY_GRAD, 1)
    ctx.set_option(KLT_OPT_L0_LEAN_FORM, _header_default_form())
    ctx._sigma_key = ctx._params_key = None              # the next configure sends its own taps again


def _built(ctx, a, n, lazy, form, what):
    ctx.build_pyramids_batch(list(range(n)), sync=True)
    code, lean_form = ae.expected(a, lazy, form)
    got = (ctx.level0_path()[0], ctx.level0_lean_form())
    assert got == (code, lean_form), "%s, KLT_OPT_L0_LAZY_GRAD %d, KLT_OPT_L0_LEAN_FORM %d: klt_level0_path / klt_level0_lean_form say %r, the case was " \
                                     "written for %r" % (what, lazy, form, got, (code, lean_form))
    assert ctx.level0_lean() == (lean_form != 0)


def _upload_and_build(ctx, a, frames, lazy=0, form=1):
    _options(ctx, a, lazy, form)
    for k, f in enumerate(frames):
        ctx.upload(k, f)
    _built(ctx, a, len(frames), lazy, form, "uploaded frames")


@pytest.mark.parametrize("name", [a.name for a in ae.ADOPT_L0])
def test_level0_case(ctx, name):
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.backend import _dp
    (a,) = [a for a in ae.ADOPT_L0 if a.name == name]
    c = a.case
    fr = list(ae.case_frames(name))
    n, shape = len(fr), (c.nrows, c.ncols)
    ko.set_threads(8)
    try:
        want = {k: ae.oracle_planes(a, fr[k]) for k in ae.ORACLE_FRAMES}
    finally:
        ko.set_threads(1)
    clip = Clip(ctx, fr)
    try:
        assert sorted({x % 4 for x in clip.addr}) == [0, 1, 2, 3] and [clip.addr[k] % 4 for k in ae.ORACLE_FRAMES] == [0, 1, 2, 3]
        ctx.configure(tc_of(c))
        if a.no_elision:
            g, d = ae.grad_taps(a)
            assert ctx._lib.klt_set_kernels(ctx._h, 2, _dp(g), len(g), _dp(d), len(d)) == 0
        # the same frames uploaded: a full build, against the oracle
        _upload_and_build(ctx, a, fr)
        up = [_planes(ctx, k, c.levels) for k in range(n)]
        for k in want:
            for l in range(c.levels):
                for p in range(3):
                    _same("uploaded frames against the oracle", up[k][l][p], want[k][l][p], k, l, p)
        # ... and adopted where they lie.  Lean shapes: a full build (the banded shapes: both streaming geometries' full kernels), then
        # the two lean forms; each after a full build of the uploaded frames in reversed order, so that every buffer of the slots holds
        # other pixels when the adopted build starts
        runs = [(0, 1)] if not a.lean else ([(0, 1)] if a.lean == "banded" else []) + [(2, 0), (2, 1)]
        for lazy, form in runs:
            _upload_and_build(ctx, a, fr[::-1])
            clip.adopt(shape)
            _options(ctx, a, lazy, form)
            what = "adopted frames (KLT_OPT_L0_LAZY_GRAD %d, KLT_OPT_L0_LEAN_FORM %d)" % (lazy, form)
            _built(ctx, a, n, lazy, form, what)
            for k in range(n):
                tag = "%s, residue %d, against the uploaded build" % (what, clip.addr[k] % 16)
                # a lean build: the image of level 0 and the levels above first, then the level-0 gradients (the records made on demand)
                order = [(l, p) for l in range(c.levels) for p in range(3) if (l, p) not in ((0, 1), (0, 2))] + [(0, 1), (0, 2), (0, 0)]
                for l, p in order:
                    got = ctx.download_level(k, p, l)
                    _same(tag, got, up[k][l][p], k, l, p)
                    if k in want:
                        _same(what + " against the oracle", got, want[k][l][p], k, l, p)
        clip.assert_untouched()
    finally:
        _restore(ctx)
        for k in range(n):
            ctx.slot_free(k)
        clip.free()


# ------------------------------------------------------------------------------------------------- the selection on the raw frame
SELECT_RESIDUES = (0, 1, 2, 3, 7)


@pytest.mark.parametrize("smooth", [True, False], ids=["smoothed", "raw"])
def test_raw_frame_selection(ctx, img0, cfg1, smooth):
    """klt_select with use_pyramid = 0 on a 320 x 240 frame adopted at five residues: with smoothBeforeSelecting the fused
    smooth-and-gradient launch of one frame reads it, without it launch_hconv_u8; the list of every residue is the uploaded slot's record for
    record, and under the cfg-1 parameters the golden one"""
    tc = make_tc(max_residue=10.0) if smooth else make_tc(max_residue=10.0, smoothBeforeSelecting=False)
    assert bool(tc.smoothBeforeSelecting) == smooth
    clip = Clip(ctx, [img0] * len(SELECT_RESIDUES), SELECT_RESIDUES)
    try:
        assert [x % 16 for x in clip.addr] == list(SELECT_RESIDUES)
        ctx.configure(tc)
        up_slot = len(SELECT_RESIDUES)
        ctx.upload(up_slot, img0)
        want, placed_want = ctx.select(up_slot, 100, use_pyramid=False)
        assert placed_want == 100
        if smooth:
            assert np.array_equal(want["x"].astype(np.float64), cfg1["sel100_x"]) and np.array_equal(want["y"].astype(np.float64), cfg1["sel100_y"])
            assert np.array_equal(want["val"].astype(np.int64), cfg1["sel100_val"])
        else:
            assert not np.array_equal(want["x"].astype(np.float64), cfg1["sel100_x"])       # the two settings select different features
        clip.adopt(img0.shape)
        for k, r in enumerate(SELECT_RESIDUES):
            got, placed = ctx.select(k, 100, use_pyramid=False)
            assert placed == placed_want and got.tobytes() == want.tobytes(), "residue %d: the list differs from the uploaded slot's" % r
        clip.assert_untouched()
    finally:
        for k in range(len(SELECT_RESIDUES) + 1):
            ctx.slot_free(k)
        clip.free()


# ------------------------------------------------------------------------------------------------------------------------- describe
DESCRIBE_RESIDUES = (1, 2, 3, 5, 15)


@pytest.mark.parametrize("shape", [(37, 41), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_describe(ctx, shape):
    """klt_describe in both modes on frames adopted at residues 1, 2, 3, 5 and 15 (describe_kernel cuts its 4-byte pieces on the address):
    the rule's records byte for byte"""
    ncols, nrows = shape
    rng = np.random.default_rng(ncols * 100 + nrows + 7)
    frames = [de.random_frame(rng, ncols, nrows, "random") for _ in DESCRIBE_RESIDUES]
    feats = edge_features(ncols, nrows)
    clip = Clip(ctx, frames, DESCRIBE_RESIDUES)
    try:
        assert [x % 16 for x in clip.addr] == list(DESCRIBE_RESIDUES)
        clip.adopt((nrows, ncols))
        for mode in (de.UPRIGHT, de.STEERED):
            ctx.set_descriptor_params(mode)
            for k, r in enumerate(DESCRIBE_RESIDUES):
                got, want = ctx.describe(k, feats).view(de.DESC_DTYPE), de.describe(frames[k], feats, mode)
                assert got.dtype == de.DESC_DTYPE and got.shape == want.shape
                bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
                assert not bad, "residue %d, mode %d: %d of %d records differ; first %d: %r, the rule says %r" % (
                    r, mode, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])
        clip.assert_untouched()
    finally:
        ctx.set_descriptor_params()
        for k in range(len(DESCRIBE_RESIDUES)):
            ctx.slot_free(k)
        clip.free()


# -------------------------------------------------------------------------------------------- a stage in front, then switched off
STAGE_NC, STAGE_NR, STAGE_N, STAGE_LEVELS, STAGE_SS = 132, 90, 16, 2, 4


def test_mixed_with_stages(ctx, plain):
    """sixteen frames at residues k % 16 behind the CLAHE stage (the level-0 kernel reads the library's aligned copies), then the stage
    switched off and the same slots built again WITHOUT a new adoption: that build reads the caller's frames where they lie, and its
    planes are those of the frames uploaded to a context that never had a stage"""
    tc = make_tc(levels=STAGE_LEVELS, ss=STAGE_SS)
    raw = [ie.slot_frame(STAGE_NC, STAGE_NR, 300 + k) for k in range(STAGE_N)]
    equalised = [ee.clahe(f, 3, 2, 768) for f in raw]
    code = expected_path(STAGE_NC, STAGE_NR, STAGE_N, False, STAGE_LEVELS, STAGE_SS, tc.smooth_sigma_fact)

    def plain_planes(frames):
        for k, f in enumerate(frames):
            plain.upload(k, f)
        plain.build_pyramids_batch(list(range(STAGE_N)), sync=True)
        assert plain.level0_path() == code
        return [_planes(plain, k, STAGE_LEVELS) for k in range(STAGE_N)]

    clip = Clip(ctx, raw)
    try:
        assert STAGE_NC % 4 == 0 and [x % 16 for x in clip.addr] == list(range(16))
        for c in (ctx, plain):
            c.configure(tc)
            c.set_option(OPT_L0_LAZY_GRAD, 0)
        ctx.set_equalize_params(mode=1, tiles_x=3, tiles_y=2, clip_q8=768)
        clip.adopt((STAGE_NR, STAGE_NC))
        for stage_on, frames in ((True, equalised), (False, raw)):
            if not stage_on:
                ctx.set_equalize_params()
            ctx.build_pyramids_batch(list(range(STAGE_N)), sync=True)
            assert bool(ctx.equalize_path()) == stage_on and ctx.level0_path() == code
            want = plain_planes(frames)
            for k in range(STAGE_N):
                if stage_on:
                    assert np.array_equal(ctx.download_equalized(k, STAGE_NC, STAGE_NR), equalised[k]) and not np.array_equal(equalised[k], raw[k])
                for l in range(STAGE_LEVELS):
                    for p in range(3):
                        _same("CLAHE %s, residue %d" % ("on" if stage_on else "switched off", k), ctx.download_level(k, p, l), want[k][l][p], k, l, p)
        clip.assert_untouched()
    finally:
        ctx.set_equalize_params()
        for c in (ctx, plain):
            c.set_option(OPT_L0_LAZY_GRAD, 1)
            for k in range(STAGE_N):
                c.slot_free(k)
        clip.free()
