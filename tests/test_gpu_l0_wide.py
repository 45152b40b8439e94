"""KLT_OPT_L0_STREAM 2: the streaming level-0 kernel on 128-column strips in 16-row bands (smooth_grad_stream<..., 128, 16>).  Every case
builds one batch of 32 DISTINCT frames under the values 2, 1 and 0 of the option, asserts through klt_level0_path that value 2 launched
the wide kernel (a case that fell back to the narrow strips or to the tile fails) and that 1 and 0 launched what tests/pyramid_expected.py
plans for them, compares all three planes of level 0 and of level 1 of EVERY frame between the three builds, and those of frames 0, 1, 15
and 31 with the CPU oracle -- bit for bit, no tolerances.

Shapes.  The frame widths sit around the 128-column strip edge and the reflect map (256, 257, 260, 383, 384, and 278 = 256 + 4 * 5 + 2:
the last surviving reduction column 4 x + 2 = 274 is the first of a pair of which the second is cut); the frame heights around the
16-row band and the segment (SEG_H - 1, SEG_H, SEG_H + 1, SEG_H + 15, SEG_H + 16, SEG_H + 17, 2 SEG_H + 3).  The wide kernel is taken
where the launch has >= 2048 workgroups (128-column strips x SEG_H-row segments x frames), and a launch holds at most 32 frames: so the
batch is 32 everywhere, a listed width comes with the fewest whole segments (plus a remainder, a different one each) that reach the
bound, and a listed height with the fewest strips (the last one cut differently each time).  They are the smallest frames the
production launch rule sends to the wide kernel; no experiment hook is set."""
import os
import re

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, TALL_PIXELS, expected_path, first_difference, frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_WIDE, STREAM_WIDE_NO_CENTRE = 7, 8       # klt_level0_path: KLT_L0_STREAM_WIDE*
WIDE_STRIP, WIDE_BAND, SEG_H = 128, 16, 128     # the wide geometry and its segment height (plan_level0 in l0_plan.h)
WIDE_WORKGROUPS = 2048                          # its grid bound
ROW_HALO = 7                                    # rows a segment reads beyond each end with 9 smoothing taps (3 + 4)
LEVELS, SS = 2, 4
ORACLE_FRAMES = (0, 1, 15, 31)


def wide_grid(ncols, nrows, batch=MAX_BATCH):
    return -(-ncols // WIDE_STRIP) * -(-nrows // SEG_H) * batch


def takes_wide(ncols, nrows, batch=MAX_BATCH):
    """the host's rule for value 2 (plan_level0, l0_plan.h): the fused reduction's own conditions, two wide strips, the grid bound"""
    hred = ncols * nrows * batch >= TALL_PIXELS and nrows >= 64 and ncols >= 64
    return hred and ncols >= 2 * WIDE_STRIP and wide_grid(ncols, nrows, batch) >= WIDE_WORKGROUPS


def _rows_for(ncols, q):
    """the fewest segments (+ a remainder of q rows) at which 32 frames of `ncols` columns reach the grid bound"""
    segs = -(-WIDE_WORKGROUPS // (-(-ncols // WIDE_STRIP) * MAX_BATCH))
    return SEG_H * segs if q == 0 else SEG_H * (segs - 1) + q


def _cols_for(nrows, r):
    """the fewest strips (the last one r columns wide; 0: whole) at which 32 frames of `nrows` rows reach the grid bound"""
    strips = -(-WIDE_WORKGROUPS // (-(-nrows // SEG_H) * MAX_BATCH))
    return WIDE_STRIP * strips if r == 0 else WIDE_STRIP * (strips - 1) + r


WIDTHS = [256, 257, 260, 383, 384, 278]
HEIGHTS = [SEG_H - 1, SEG_H, SEG_H + 1, SEG_H + 15, SEG_H + 16, SEG_H + 17, 2 * SEG_H + 3]
# (ncols, nrows, sigma): the widths with row remainders 0, 1, 5, 16, 17, 127; the heights with last strips of 0, 4, 1, 126, 16, 2 and 127 columns;
# sigma 0.1 / 0.2 = 5 / 9 smoothing taps, alternating
WIDTH_SHAPES = [(nc, _rows_for(nc, q), s) for nc, q, s in zip(WIDTHS, [0, 1, 5, 16, 17, SEG_H - 1], [0.1, 0.2, 0.1, 0.2, 0.1, 0.2])]
HEIGHT_SHAPES = [(_cols_for(nr, r), nr, s) for nr, r, s in zip(HEIGHTS, [0, 4, 1, 126, 16, 2, 127], [0.2, 0.1, 0.2, 0.1, 0.2, 0.1, 0.2])]
SHAPES = WIDTH_SHAPES + HEIGHT_SHAPES
# ... and the other tap count where an edge kind (edge_kinds below) would else be seen with one tap count only
OTHER_TAPS = [(nc, nr, {0.1: 0.2, 0.2: 0.1}[s]) for nc, nr, s in (WIDTH_SHAPES[0], WIDTH_SHAPES[1], WIDTH_SHAPES[5], HEIGHT_SHAPES[0], HEIGHT_SHAPES[4])]
# u8 frames whose derivative taps forbid the centre-tap elision, 5 and 9 smoothing taps
NO_ELISION = [WIDTH_SHAPES[2], (WIDTH_SHAPES[3][0], WIDTH_SHAPES[3][1], 0.1), HEIGHT_SHAPES[2], (HEIGHT_SHAPES[5][0], HEIGHT_SHAPES[5][1], 0.2)]


def shape_id(s):
    return "%dx%d-s%.1f" % s


def edge_kinds(ncols, nrows):
    """which edges of the wide geometry fall inside a frame of this size (the not-gpu test below asserts that the list has them all)"""
    kinds = set()
    r, q = ncols % WIDE_STRIP, nrows % SEG_H
    kinds.add("last strip whole" if r == 0 else "last strip cut, unaligned" if ncols % 4 else "last strip cut, aligned")
    if r and r < 16:
        kinds.add("last strip narrower than the column halo")
    if nrows > SEG_H:
        kinds.add("prologue inside the frame")
    kinds.add("one segment" if nrows <= SEG_H else "last segment whole" if q == 0 else "last segment cut")
    if q and q <= ROW_HALO:
        kinds.add("last segment inside the row halo")
    if q % WIDE_BAND:
        kinds.add("last band cut")
    if q % WIDE_BAND == 1:
        kinds.add("last band of one row")
    if q % WIDE_BAND == WIDE_BAND - 1:
        kinds.add("last band one row short")
    if q and q % WIDE_BAND == 0:
        kinds.add("last segment of whole bands")
    return kinds


EDGE_KINDS = ["last strip whole", "last strip cut, unaligned", "last strip cut, aligned", "last strip narrower than the column halo",
              "prologue inside the frame", "one segment", "last segment whole", "last segment cut", "last segment inside the row halo",
              "last band cut", "last band of one row", "last band one row short", "last segment of whole bands"]


# ------------------------------------------------------------------------------------------------------------------------ expected planes
def _tc(sigma):
    return make_tc(levels=LEVELS, ss=SS, smooth_sigma_fact=sigma)


def unelidable_grad_taps(sigma):
    """the gradient taps of the default sigma with the derivative's centre tap -0.0 instead of +0.0: the host then keeps the centre
    product (l0_deriv_centre_elidable, l0_plan.h, wants the bits of +0.0)"""
    from pyfeaturetrack_amd.params import taps_from_params
    g, d = taps_from_params(params_from_tc(_tc(sigma)))[2]
    d = list(d)
    assert d[len(d) // 2] == 0.0
    d[len(d) // 2] = -0.0
    return list(g), d


def oracle_planes(frame, sigma, grad_taps=None):
    """[level][plane] of the CPU oracle.  grad_taps = (gauss, deriv): the gradients of every level from these taps instead of the ones the
    oracle makes from the gradient sigma (gradx = derivative along x then Gaussian along y, grady the other way round, as ko_gradients)"""
    from oracle import klt_oracle as ko
    p = ko.Pyramids(params_from_tc(_tc(sigma)), np.asarray(frame, np.float32))
    out = [[p.level(w, l) for w in range(3)] for l in range(LEVELS)]
    if grad_taps is not None:
        g, d = grad_taps
        out = [[img, ko.convolve_separate(img, d, g), ko.convolve_separate(img, g, d)] for img, _, _ in out]
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the trial
@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def run_wide_trial(ctx, ncols, nrows, sigma, f32, no_elision=False, batch=MAX_BATCH, oracle_frames=ORACLE_FRAMES):
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.backend import _dp
    fr = frames((nrows, ncols), batch, f32, ncols * 65536 + nrows)
    grad_taps = unelidable_grad_taps(sigma) if no_elision else None
    ko.set_threads(8)
    try:
        want = {k: oracle_planes(fr[k], sigma, grad_taps) for k in oracle_frames if k < batch}
    finally:
        ko.set_threads(1)
    ctx.configure(_tc(sigma))
    first = None
    try:
        if no_elision:
            g, d = grad_taps
            assert ctx._lib.klt_set_kernels(ctx._h, 2, _dp(g), len(g), _dp(d), len(d)) == 0
        ctx.set_option(OPT_FUSED_KERNELS, 1)
        ctx.set_option(OPT_FUSED_HREDUCE, 1)
        for opt in (2, 1, 0):
            ctx.set_option(OPT_L0_STREAM, opt)
            for k, f in enumerate(fr):
                ctx.upload(k, f)
            ctx.build_pyramids_batch(list(range(batch)), sync=True)
            code = ctx.level0_path()[0]
            if opt == 2:
                want_code = STREAM_WIDE if f32 or no_elision else STREAM_WIDE_NO_CENTRE
            else:
                want_code = expected_path(ncols, nrows, batch, f32 or no_elision, LEVELS, SS, sigma, stream_opt=opt)[0]
            assert code == want_code, "KLT_OPT_L0_STREAM %d: klt_level0_path says %d, the case was written for %d" % (opt, code, want_code)
            planes = [[[ctx.download_level(k, p, l) for p in range(3)] for l in range(LEVELS)] for k in range(batch)]
            for k in range(batch):
                for l in range(LEVELS):
                    for p in range(3):
                        bad = first_difference(planes[k][l][p], want[k][l][p]) if k in want else None
                        against = "the oracle"
                        if not bad and first is not None:
                            bad, against = first_difference(planes[k][l][p], first[k][l][p]), "the build with value 2"
                        assert not bad, "KLT_OPT_L0_STREAM %d: frame %d of %d, plane %d of level %d against %s: %s" % (opt, k, batch, p, l, against, bad)
            if first is None:
                first = planes
    finally:
        ctx.set_option(OPT_L0_STREAM, 2)                 # (the default)
        ctx._sigma_key = ctx._params_key = None          # the next configure sends its own taps again


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", SHAPES + OTHER_TAPS, ids=shape_id)
def test_wide_shape(ctx, shape, f32):
    """u8 frames (centre tap elided) and f32 frames at every listed width and height"""
    run_wide_trial(ctx, *shape, f32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NO_ELISION, ids=shape_id)
def test_wide_u8_centre_product_kept(ctx, shape):
    """u8 frames with a derivative centre tap of -0.0: smooth_grad_stream<u8, NS, false, 128, 16>, the oracle's gradients from the same taps"""
    run_wide_trial(ctx, *shape, False, no_elision=True)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
def test_wide_batch_frames_differ(ctx, f32):
    """blockIdx.z addressing: 32 frames that all differ, EVERY one of them against the oracle's planes of its own frame"""
    nc = 384
    run_wide_trial(ctx, nc, _rows_for(nc, 0), 0.1, f32, oracle_frames=tuple(range(MAX_BATCH)))


# ------------------------------------------------------------------------------------------------------------------------------- no GPU
def test_shape_list_puts_every_edge_inside_a_frame():
    """the constants above are the kernel's; every shape takes the wide kernel under the host's rule at 32 frames and not one segment or
    strip smaller; the widths and heights are the listed ones; together the shapes have an edge of every kind -- last strip, last band,
    last segment, prologue -- inside a frame, with 5 and with 9 smoothing taps"""
    src = open(os.path.join(REPO, "pyfeaturetrack_amd", "csrc", "l0_plan.h")).read()
    assert re.search(r"L0W_TW = (\d+), L0W_SB = (\d+)", src).groups() == (str(WIDE_STRIP), str(WIDE_BAND))
    assert re.search(r"L0W_MIN_WGS = (\d+)", src).group(1) == str(WIDE_WORKGROUPS)
    assert re.search(r"shw = seg_of\(L0W_SB, (\d+)\)", src).group(1) == str(SEG_H) and SEG_H % WIDE_BAND == 0
    hdr = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    assert re.search(r"#define\s+KLT_L0_STREAM_WIDE\s+(\d+)", hdr).group(1) == str(STREAM_WIDE)
    assert re.search(r"#define\s+KLT_L0_STREAM_WIDE_NO_CENTRE\s+(\d+)", hdr).group(1) == str(STREAM_WIDE_NO_CENTRE)
    assert [s[0] for s in WIDTH_SHAPES] == [256, 257, 260, 383, 384, 278] and WIDTHS[5] % 4 == 2
    assert [s[1] for s in HEIGHT_SHAPES] == [SEG_H - 1, SEG_H, SEG_H + 1, SEG_H + 15, SEG_H + 16, SEG_H + 17, 2 * SEG_H + 3]
    for nc, nr, sigma in SHAPES + OTHER_TAPS + NO_ELISION:
        assert takes_wide(nc, nr) and not takes_wide(nc, nr, MAX_BATCH - 1), (nc, nr)
        assert nc * nr * MAX_BATCH <= 36000000, (nc, nr)
    assert all(not takes_wide(nc, nr - SEG_H) for nc, nr, _ in WIDTH_SHAPES) and all(not takes_wide(nc - WIDE_STRIP, nr) for nc, nr, _ in HEIGHT_SHAPES)
    for sigma in (0.1, 0.2):
        seen = set().union(*(edge_kinds(nc, nr) for nc, nr, s in SHAPES + OTHER_TAPS if s == sigma))
        assert seen == set(EDGE_KINDS), (sigma, sorted(set(EDGE_KINDS) - seen))
    assert {s for _, _, s in NO_ELISION} == {0.1, 0.2}


def test_oracle_makes_the_expected_planes_of_every_shape():
    """no GPU: the oracle builds both levels of a frame of every listed shape (u8 and f32 draws), and the gradients recomputed from
    explicit taps -- what the cases without the elision compare with -- are the oracle's own when the taps are its own"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.params import taps_from_params
    ko.set_threads(8)
    try:
        for nc, nr, sigma in SHAPES:
            for f32 in (False, True):
                fr = frames((nr, nc), 1, f32, nc * 65536 + nr)[0]
                planes = oracle_planes(fr, sigma)
                assert [p.shape for p in planes[0]] == [(nr, nc)] * 3 and [p.shape for p in planes[1]] == [(nr // SS, nc // SS)] * 3
                assert all(np.isfinite(p).all() for lv in planes for p in lv)
        nc, nr, sigma = NO_ELISION[0]
        fr = frames((nr, nc), 1, False, 3)[0]
        g, d = taps_from_params(params_from_tc(_tc(sigma)))[2]
        own, again = oracle_planes(fr, sigma), oracle_planes(fr, sigma, (list(g), list(d)))
        assert all(first_difference(a, b) is None for lo, la in zip(own, again) for a, b in zip(lo, la))
        changed = oracle_planes(fr, sigma, unelidable_grad_taps(sigma))
        assert all(np.array_equal(a, b) for lo, lc in zip(own, changed) for a, b in zip(lo, lc))       # (equal as numbers; zeros may change sign)
    finally:
        ko.set_threads(1)
