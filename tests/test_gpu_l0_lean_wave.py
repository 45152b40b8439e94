"""KLT_OPT_L0_LEAN_FORM: the wave form of the lean level-0 kernel (smooth_grad_lean_wave: a wavefront owns a 232-column strip and walks it
down a segment of rows on its own) against the banded lean form, the full build and the CPU oracle.

Every plane case builds one batch of 32 DISTINCT frames three times -- full (KLT_OPT_L0_LAZY_GRAD 0), lean with form 0 (banded) and lean
with form 1 (wave), each lean build after a full build of the same frames in reversed slot order (the record buffers then hold other
pixels than the ones to be made on demand) -- asserts klt_level0_lean_form = 0, 1 and 2 for the three, and compares, bit for bit and without tolerances, for both
lean builds:
  * the image plane of level 0 and all three planes of level 1 of EVERY frame with the full build's, and those of frames 0, 1, 15 and 31
    with the CPU oracle's;
  * after the downloads of gradx and grady, all three planes of level 0 in the same way.

Shapes: the smallest frames the production rule (default KLT_OPT_L0_STREAM) sends lean at 32 frames -- a streaming geometry with >= 2048
workgroups, wide (128-column strips, 128-row segments) or, where those miss the bound, narrow (64 / 160) -- derived as
tests/test_gpu_l0_lean.py derives them, but for the wave kernel's edges:
  * widths whose last 232-column strip is whole, 4, 1 and 230 columns wide (two strips or more, >= 256 columns) and two widths with
    ncols % 4 = 1 and 2 (every strip then reads element by element), each with the fewest rows that reach the bound;
  * heights whose last segment is SEG - 1, 1, NS - 2 (shorter than the vertical window) and 3 rows high: SEG - 1, SEG + 1 and SEG + NS - 2
    on top of two whole segments (the fused reduction, which every lean launch has, asks for >= 64 rows) and 2 SEG + 3, each with the
    fewest columns that reach the bound, rounded up to a multiple of 4 so that the interior strips take the aligned path.
SEG and the strip width are pyfeaturetrack_amd._abi's figures, which a CPU test holds against the header's and the kernel's.
u8 and f32 frames; 5 and 9 smoothing taps (sigma 0.1 / 0.2) alternate over the shapes and swap between the two input types, so every
width kind and every height kind sees both."""
import os
import re

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, first_difference, frames
from pyfeaturetrack_amd._abi import KLT_OPT_L0_LEAN_FORM, L0_LEAN_WAVE_COLS as STRIP, L0_LEAN_WAVE_SEG as SEG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_L0_LAZY_GRAD = 22
WORKGROUPS = 2048                                # the grid bound of both banded geometries
BANDED = ((128, 128, 256), (64, 160, 128))       # strip, segment, fewest columns: wide, then narrow (plan_level0's order)
LEVELS, SS = 2, 4
ORACLE_FRAMES = (0, 1, 15, 31)
TAPS = {0.1: 5, 0.2: 9}
TRACK_N = 128                                    # features per pair: 16 pairs x 128 = 2048, the shortest launch with a lazy form
WIDTH_LAST = (0, 4, 1, 230)                      # columns of the last strip (0: whole)
WIDTH_MOD4 = (2 * STRIP + 13, 2 * STRIP + 26)    # ncols % 4 = 1 and 2


def goes_lean(ncols, nrows, batch=MAX_BATCH):
    """the host's rule for a lean launch at the default KLT_OPT_L0_STREAM (plan_level0, l0_plan.h: the fused reduction, a streaming geometry)"""
    hred = ncols * nrows * batch >= 1000000 and nrows >= 64 and ncols >= 64
    return hred and any(ncols >= least and -(-ncols // strip) * -(-nrows // seg) * batch >= WORKGROUPS for strip, seg, least in BANDED)


def takes_wave(ncols, nrows, ntaps):
    """... and for the wave form of it (plan_level0 again)"""
    return ncols >= 256 and nrows >= ntaps


def _fewest(ok, start):
    n = start
    while not ok(n):
        n += 1
    return n


def shapes():
    """(kind, ncols, nrows, sigma for u8 frames): six widths, four heights (the third once per tap count)"""
    out = []
    widths = [2 * STRIP if r == 0 else (2 * STRIP + r if STRIP + r < 256 else STRIP + r) for r in WIDTH_LAST] + list(WIDTH_MOD4)
    for i, nc in enumerate(widths):
        out.append(("w", nc, _fewest(lambda nr: goes_lean(nc, nr), 64), (0.1, 0.2)[i % 2]))
    rows = {"seg-1": lambda nt: 3 * SEG - 1, "seg+1": lambda nt: 3 * SEG + 1, "seg+ns-2": lambda nt: 3 * SEG + nt - 2, "2seg+3": lambda nt: 2 * SEG + 3}
    # (the third height belongs to a tap count: one frame size for each, which both input types keep -- kind "h*")
    for q, kind, sigma in (("seg-1", "h", 0.2), ("seg+1", "h", 0.1), ("seg+ns-2", "h*", 0.2), ("seg+ns-2", "h*", 0.1), ("2seg+3", "h", 0.2)):
        nr = rows[q](TAPS[sigma])
        nc = _fewest(lambda n: goes_lean(n, nr), 2 * STRIP)
        out.append((kind, -(-nc // 4) * 4, nr, sigma))
    return out


def _sigma(case, f32):
    """the taps swap between the input types, except where the height belongs to one tap count"""
    kind, _, _, sigma = case
    return sigma if (not f32 or kind == "h*") else (0.1, 0.2)[sigma == 0.1]


CASES = shapes()


def case_id(c):
    return "%s-%dx%d-s%.1f" % c


def _tc(sigma):
    return make_tc(levels=LEVELS, ss=SS, smooth_sigma_fact=sigma)


def oracle_planes(frame, sigma):
    from oracle import klt_oracle as ko
    p = ko.Pyramids(params_from_tc(_tc(sigma)), np.asarray(frame, np.float32))
    return [[p.level(w, l) for w in range(3)] for l in range(LEVELS)]


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _setup(ctx, sigma):
    ctx.configure(_tc(sigma))
    ctx.set_option(OPT_FUSED_KERNELS, 1)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, 2)


def _header_default_form():
    hdr = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    return int(re.search(r"#define\s+KLT_L0_LEAN_FORM_DEFAULT\s+(\d+)", hdr).group(1))


def _restore(ctx):
    ctx.set_option(OPT_L0_LAZY_GRAD, 1)              # (the defaults)
    ctx.set_option(KLT_OPT_L0_LEAN_FORM, _header_default_form())


def _build(ctx, fr, lazy, form, want_form):
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)
    ctx.set_option(KLT_OPT_L0_LEAN_FORM, form)
    for k, f in enumerate(fr):
        ctx.upload(k, f)
    ctx.build_pyramids_batch(list(range(len(fr))), sync=True)
    got = ctx.level0_lean_form()
    assert got == want_form, "KLT_OPT_L0_LAZY_GRAD %d, KLT_OPT_L0_LEAN_FORM %d: klt_level0_lean_form says %d" % (lazy, form, got)
    assert ctx.level0_lean() == (want_form != 0)


def _compare(what, got, full, want, k, l, p):
    bad = first_difference(got, want[k][l][p]) if k in want else None
    against = "the oracle"
    if not bad:
        bad, against = first_difference(got, full[k][l][p]), "the full build"
    assert not bad, "%s: frame %d, plane %d of level %d against %s: %s" % (what, k, p, l, against, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wave_build_planes(ctx, case, f32):
    from oracle import klt_oracle as ko
    _, ncols, nrows, _ = case
    sigma = _sigma(case, f32)
    batch = MAX_BATCH
    fr = frames((nrows, ncols), batch, f32, ncols * 65536 + nrows)
    ko.set_threads(8)
    try:
        want = {k: oracle_planes(fr[k], sigma) for k in ORACLE_FRAMES}
    finally:
        ko.set_threads(1)
    _setup(ctx, sigma)
    try:
        _build(ctx, fr, 0, 1, 0)
        full = [[[ctx.download_level(k, p, l) for p in range(3)] for l in range(LEVELS)] for k in range(batch)]
        for k in want:
            for l in range(LEVELS):
                for p in range(3):
                    bad = first_difference(full[k][l][p], want[k][l][p])
                    assert not bad, "full build: frame %d, plane %d of level %d against the oracle: %s" % (k, p, l, bad)
        for form, want_form, name in ((0, 1, "banded lean build"), (1, 2, "wave lean build")):
            _build(ctx, fr[::-1], 0, 1, 0)                   # slot k holds frame 31 - k: the record buffers hold other pixels when the lean build starts
            _build(ctx, fr, 2, form, want_form)
            for k in range(batch):
                _compare(name, ctx.download_level(k, 0, 0), full, want, k, 0, 0)
                for p in range(3):
                    _compare(name, ctx.download_level(k, p, 1), full, want, k, 1, p)
            for k in range(batch):
                gx, gy = ctx.download_level(k, 1, 0), ctx.download_level(k, 2, 0)
                for p, got in enumerate((ctx.download_level(k, 0, 0), gx, gy)):
                    _compare(name + ", records made on demand", got, full, want, k, 0, p)
    finally:
        _restore(ctx)


def _small_case():
    return min(CASES, key=lambda c: c[1] * c[2])


@pytest.mark.gpu
def test_build_and_track_equal_under_both_forms_and_the_oracle(ctx):
    """sixteen pairs x 128 features (2048: the shortest lazy tracker launch) on the smallest shape: the records after build-and-track
    under form 0 and under form 1 are equal, and both are the oracle's"""
    from benchlib.common import oracle_track
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    case = _small_case()
    _, ncols, nrows, sigma = case
    npairs = MAX_BATCH // 2
    fr = frames((nrows, ncols), MAX_BATCH, False, 91)
    rng = np.random.default_rng([91, 5])
    lists = []
    for i in range(npairs):
        fl = np.zeros(TRACK_N, FEAT_DTYPE)
        fl["x"] = rng.uniform(4, ncols - 4, TRACK_N).astype(np.float32)      # (up to the frame's edge: strips 0 and the last, rows 0.. and ..nrows)
        fl["y"] = rng.uniform(4, nrows - 4, TRACK_N).astype(np.float32)
        lists.append(fl)
    _setup(ctx, sigma)
    try:
        recs = {}
        for form, want_form in ((0, 1), (1, 2)):
            for i, fl in enumerate(lists):
                ctx.featbuf_upload(100 + i, fl)
            _build(ctx, fr, 2, form, want_form)
            ctx.track_batch_async([(2 * i, 2 * i + 1, 100 + i, 200 + i) for i in range(npairs)], TRACK_N)
            ctx.sync()
            assert ctx.level0_lean_form() == want_form
            recs[form] = [ctx.featbuf_download(200 + i, TRACK_N) for i in range(npairs)]
        p = params_from_tc(_tc(sigma))
        for i in range(npairs):
            assert recs[0][i].tobytes() == recs[1][i].tobytes(), "pair %d: the records differ between the two lean forms" % i
            want = oracle_track(ko, p, fr[2 * i], fr[2 * i + 1], lists[i], threads=8)
            assert np.array_equal(recs[1][i]["val"], want["val"]), "pair %d: status words differ from the oracle's" % i
            for k in ("x", "y"):
                assert np.array_equal(recs[1][i][k], want[k].astype(np.float32)), "pair %d: %s differs from the oracle's" % (i, k)
    finally:
        _restore(ctx)


@pytest.mark.gpu
def test_option_round_trip(ctx):
    """form 0 is the parent's launch (the banded lean kernel), form 1 the wave kernel, and back; a full build reports 0; values other
    than 0 and 1 are refused"""
    from pyfeaturetrack_amd.backend import KltBackendError
    _, ncols, nrows, sigma = _small_case()
    fr = frames((nrows, ncols), MAX_BATCH, False, 92)
    _setup(ctx, sigma)
    try:
        _build(ctx, fr, 2, 0, 1)
        _build(ctx, fr, 2, 1, 2)
        _build(ctx, fr, 2, 0, 1)
        _build(ctx, fr, 0, 1, 0)
        with pytest.raises(KltBackendError):
            ctx.set_option(KLT_OPT_L0_LEAN_FORM, 2)
    finally:
        _restore(ctx)


# ------------------------------------------------------------------------------------------------------------------------------- no GPU
def test_case_list_and_constants():
    """the constants are the header's and the kernel's; every case goes lean under the host's rule at 32 frames and takes the wave form,
    and is the smallest that does: one row (widths) or four columns (heights) fewer, or one frame fewer, and it would not go lean; the edge
    kinds, both tap counts and both input types are all there"""
    hdr = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    src = open(os.path.join(REPO, "pyfeaturetrack_amd", "csrc", "pyramid_kernels.hip")).read()
    plan = open(os.path.join(REPO, "pyfeaturetrack_amd", "csrc", "l0_plan.h")).read()
    assert int(re.search(r"#define\s+KLT_OPT_L0_LEAN_FORM\s+(\d+)", hdr).group(1)) == KLT_OPT_L0_LEAN_FORM == 23
    assert int(re.search(r"#define\s+KLT_L0_LEAN_WAVE_SEG\s+(\d+)", hdr).group(1)) == SEG
    assert int(re.search(r"LW_COLS = (\d+), LW_HALO = 12", src).group(1)) == STRIP
    assert int(re.search(r"L0_WAVE_COLS = (\d+), L0_WAVE_WAVES = 4", plan).group(1)) == STRIP and "LW_COLS == L0_WAVE_COLS" in src
    assert re.search(r"q\.lean_form_opt == 1 && q\.uniform && q\.ncols >= 256 && q\.nrows >= q\.smooth->n\)", plan)
    assert re.search(r"L0S_MIN_WGS = (\d+), L0W_MIN_WGS = (\d+)", plan).groups() == (str(WORKGROUPS),) * 2
    assert re.search(r"L0S_TW = (\d+), L0S_SB = \d+, L0W_TW = (\d+)", plan).groups() == (str(BANDED[1][0]), str(BANDED[0][0]))
    assert re.search(r"shw = seg_of\(L0W_SB, (\d+)\), sh = seg_of\(L0S_SB, (\d+)\)", plan).groups() == (str(BANDED[0][1]), str(BANDED[1][1]))
    widths = [c for c in CASES if c[0] == "w"]
    heights = [c for c in CASES if c[0] != "w"]
    assert [(c[1] % STRIP) for c in widths[:4]] == list(WIDTH_LAST) and [c[1] % 4 for c in widths[4:]] == [1, 2]
    assert all(c[1] % 4 == 0 for c in widths[:2]) and all(c[1] % 4 == 0 for c in heights)
    assert [c[2] % SEG for c in heights] == [SEG - 1, 1, TAPS[heights[2][3]] - 2, TAPS[heights[3][3]] - 2, 3]
    assert TAPS[heights[2][3]] != TAPS[heights[3][3]]
    for c in CASES:
        _, nc, nr, _ = c
        assert -(-nc // STRIP) >= 2
        assert goes_lean(nc, nr) and not goes_lean(nc, nr, MAX_BATCH - 1), c
        assert not (goes_lean(nc, nr - 1) if c[0] == "w" else goes_lean(nc - 4, nr)), c
        for f32 in (False, True):
            assert takes_wave(nc, nr, TAPS[_sigma(c, f32)]), c
        assert nc * nr * MAX_BATCH <= 36000000, c
    for c in CASES:                                      # every width and every height sees both tap counts
        assert c[0] == "h*" or {TAPS[_sigma(c, False)], TAPS[_sigma(c, True)]} == {5, 9}
    assert TRACK_N * (MAX_BATCH // 2) == 2048
