"""KLT_OPT_L0_LAZY_GRAD: the lean form of the streaming level-0 kernels (smooth_grad_stream<..., LEAN>: no gradients, no level-0 records,
the smoothed image to the slot's compact plane) and the records made from that plane on demand (ensure_level0_records).

Every plane case builds one batch of 32 DISTINCT frames twice -- option 0 (full) and option 2 (lean wherever a streaming kernel is
launched), with a full build of the same frames in reversed slot order in between, so that the record buffers hold other pixels when the
lean build starts and records that nothing made on demand cannot pass for the right ones -- asserts through klt_level0_path that both builds launched the streaming geometry the case was written for and through
klt_level0_lean that the second one was lean, and compares, bit for bit and without tolerances:
  * the image plane of level 0 and all three planes of level 1 of EVERY frame of the lean build with the full build's, and those of
    frames 0, 1, 15 and 31 with the CPU oracle's;
  * after the downloads of gradx and grady, all three planes of level 0 in the same way.

Shapes, as tests/test_gpu_l0_wide.py derives them, for both streaming geometries (128-column strips in 16-row bands with segments of 128
rows, KLT_OPT_L0_STREAM 2; 64-column strips in 32-row bands with segments of 160 rows, KLT_OPT_L0_STREAM 1): a launch takes a streaming
kernel where it has >= 2048 workgroups (strips x segments x frames) and holds at most 32 frames, so the batch is 32, a listed width (256,
257, 278) comes with the fewest segments that reach the bound and a listed height (SEG_H - 1, SEG_H + 1, SEG_H + 17, 2 SEG_H + 3) with the
fewest strips: the smallest frames the production rule sends to each geometry.  u8 and f32 frames; 5 and 9 smoothing taps alternate over
the shapes (sigma 0.1 / 0.2), each width and each height kind with both over the two geometries.

The rule of option 1 (a slot is built lean once a tracker launch with a lazy form has read it and nothing has asked for its level-0
records since its previous build) and the failure of the new allocation site are tested on the smallest shape of each geometry."""
import os
import re

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM, first_difference, frames

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_L0_LAZY_GRAD, OPT_FAIL_ALLOC_AFTER = 22, 19
WORKGROUPS = 2048                                # the grid bound of both geometries
LEVELS, SS = 2, 4
ORACLE_FRAMES = (0, 1, 15, 31)
# name -> (KLT_OPT_L0_STREAM value, strip width, segment height, klt_level0_path codes for f32 / u8 frames)
GEOMETRIES = {"wide": (2, 128, 128, (7, 8)), "narrow": (1, 64, 160, (5, 6))}
TRACK_N = 128                                    # features per pair: 16 pairs x 128 = 2048, the shortest launch with a lazy form


def _rows_for(strip, seg, ncols, q):
    segs = -(-WORKGROUPS // (-(-ncols // strip) * MAX_BATCH))
    return seg * segs if q == 0 else seg * (segs - 1) + q


def _cols_for(strip, seg, nrows, r):
    strips = -(-WORKGROUPS // (-(-nrows // seg) * MAX_BATCH))
    return strip * strips if r == 0 else strip * (strips - 1) + r


def shapes_of(geom):
    """(ncols, nrows, sigma) of a geometry: the three widths with row remainders 0, 1 and 17, the four heights with last strips that are
    whole, 4, 1 and strip - 2 columns wide"""
    _, strip, seg, _ = GEOMETRIES[geom]
    sig = (0.1, 0.2) if geom == "wide" else (0.2, 0.1)
    widths = [(nc, _rows_for(strip, seg, nc, q), sig[i % 2]) for i, (nc, q) in enumerate(zip((256, 257, 278), (0, 1, 17)))]
    heights = [(_cols_for(strip, seg, nr, r), nr, sig[(i + 1) % 2])
               for i, (nr, r) in enumerate(zip((seg - 1, seg + 1, seg + 17, 2 * seg + 3), (0, 4, 1, strip - 2)))]
    return widths + heights


CASES = [(geom,) + s for geom in GEOMETRIES for s in shapes_of(geom)]


def case_id(c):
    return "%s-%dx%d-s%.1f" % c


def takes_geometry(geom, ncols, nrows, batch=MAX_BATCH):
    """the host's rule (plan_level0, l0_plan.h) for the geometry's own value of KLT_OPT_L0_STREAM"""
    _, strip, seg, _ = GEOMETRIES[geom]
    hred = ncols * nrows * batch >= 1000000 and nrows >= 64 and ncols >= 64
    return hred and ncols >= 2 * strip and -(-ncols // strip) * -(-nrows // seg) * batch >= WORKGROUPS


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


def _setup(ctx, geom, sigma):
    ctx.configure(_tc(sigma))
    ctx.set_option(OPT_FUSED_KERNELS, 1)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, GEOMETRIES[geom][0])


def _restore(ctx):
    ctx.set_option(OPT_L0_LAZY_GRAD, 1)              # (the defaults)
    ctx.set_option(OPT_L0_STREAM, 2)


def _build(ctx, fr, lazy, geom, f32, want_lean):
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)
    for k, f in enumerate(fr):
        ctx.upload(k, f)
    ctx.build_pyramids_batch(list(range(len(fr))), sync=True)
    code, want_code = ctx.level0_path()[0], GEOMETRIES[geom][3][0 if f32 else 1]
    assert code == want_code, "KLT_OPT_L0_LAZY_GRAD %d: klt_level0_path says %d, the case was written for %d" % (lazy, code, want_code)
    assert ctx.level0_lean() == want_lean, "KLT_OPT_L0_LAZY_GRAD %d: klt_level0_lean says %r" % (lazy, ctx.level0_lean())


def _compare(what, got, full, want, k, l, p):
    bad = first_difference(got, want[k][l][p]) if k in want else None
    against = "the oracle"
    if not bad:
        bad, against = first_difference(got, full[k][l][p]), "the full build"
    assert not bad, "%s: frame %d, plane %d of level %d against %s: %s" % (what, k, p, l, against, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lean_build_planes(ctx, case, f32):
    from oracle import klt_oracle as ko
    geom, ncols, nrows, sigma = case
    batch = MAX_BATCH
    fr = frames((nrows, ncols), batch, f32, ncols * 65536 + nrows)
    ko.set_threads(8)
    try:
        want = {k: oracle_planes(fr[k], sigma) for k in ORACLE_FRAMES}
    finally:
        ko.set_threads(1)
    _setup(ctx, geom, sigma)
    try:
        _build(ctx, fr, 0, geom, f32, False)
        full = [[[ctx.download_level(k, p, l) for p in range(3)] for l in range(LEVELS)] for k in range(batch)]
        for k in want:
            for l in range(LEVELS):
                for p in range(3):
                    bad = first_difference(full[k][l][p], want[k][l][p])
                    assert not bad, "full build: frame %d, plane %d of level %d against the oracle: %s" % (k, p, l, bad)
        _build(ctx, fr[::-1], 0, geom, f32, False)       # slot k holds frame 31 - k: the record buffers hold other pixels when the lean build starts
        _build(ctx, fr, 2, geom, f32, True)
        for k in range(batch):
            _compare("lean build", ctx.download_level(k, 0, 0), full, want, k, 0, 0)
            for p in range(3):
                _compare("lean build", ctx.download_level(k, p, 1), full, want, k, 1, p)
        for k in range(batch):
            gx, gy = ctx.download_level(k, 1, 0), ctx.download_level(k, 2, 0)
            for p, got in enumerate((ctx.download_level(k, 0, 0), gx, gy)):
                _compare("lean build, records made on demand", got, full, want, k, 0, p)
    finally:
        _restore(ctx)


def _small_case(geom):
    return min((c for c in CASES if c[0] == geom), key=lambda c: c[1] * c[2])


def _lists(ctx, ncols, nrows, npairs, seed):
    """a list of TRACK_N live features per pair in feature buffers 100 + i, inside the frame's border"""
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    rng = np.random.default_rng([seed, 5])
    for i in range(npairs):
        fl = np.zeros(TRACK_N, FEAT_DTYPE)
        fl["x"] = rng.uniform(30, ncols - 30, TRACK_N).astype(np.float32)
        fl["y"] = rng.uniform(30, nrows - 30, TRACK_N).astype(np.float32)
        ctx.featbuf_upload(100 + i, fl)


def _track_all(ctx, npairs):
    ctx.track_batch_async([(2 * i, 2 * i + 1, 100 + i, 200 + i) for i in range(npairs)], TRACK_N)
    ctx.sync()
    return [ctx.featbuf_download(200 + i, TRACK_N) for i in range(npairs)]


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_adaptive_rule(ctx, geom):
    """option 1: the first build is full; build -> plain tracker on every slot -> build is lean the second time, and that tracker's records
    on the lean slots are the ones it gave on the full ones; build -> tracker -> selection on every slot -> build is not lean"""
    _, ncols, nrows, sigma = _small_case(geom)
    npairs = MAX_BATCH // 2
    fr = frames((nrows, ncols), MAX_BATCH, False, 77)
    _setup(ctx, geom, sigma)
    try:
        ctx.set_option(OPT_L0_LAZY_GRAD, 0)
        for k in range(MAX_BATCH):                       # (a size and a build of their own: nothing an earlier case left in the slots counts)
            ctx.upload(k, fr[k][:-1])
        ctx.build_pyramids_batch(list(range(MAX_BATCH)), sync=True)
        _lists(ctx, ncols, nrows, npairs, 1)
        _build(ctx, fr, 1, geom, False, False)           # first build of this size: full
        first = _track_all(ctx, npairs)
        _build(ctx, fr, 1, geom, False, True)            # read by a tracker with a lazy form, nothing asked for the records: lean
        again = _track_all(ctx, npairs)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes(), "the tracker on lean slots gave other records than on full ones"
        _build(ctx, fr, 1, geom, False, True)            # ... and stays lean
        _track_all(ctx, npairs)
        for k in range(MAX_BATCH):
            ctx.select(k, 64, use_pyramid=True)
        _build(ctx, fr, 1, geom, False, False)           # a selection asked for the records of every slot: full
        third = _track_all(ctx, npairs)
        for a, b in zip(first, third):
            assert a.tobytes() == b.tobytes()
    finally:
        _restore(ctx)


@pytest.mark.gpu
def test_compact_plane_allocation_failure(ctx):
    """the one new allocation site (a slot's compact level-0 plane, on its first lean build): refused, the build answers KLT_ERR_NOMEM and
    the context stays usable -- the same build then goes through, lean, with the planes of the full build"""
    from pyfeaturetrack_amd.backend import Context, KltOutOfMemory
    geom, ncols, nrows, sigma = _small_case("wide")
    fr = frames((nrows, ncols), MAX_BATCH, False, 78)
    own = Context(0)                                     # (slots that have never been built lean)
    try:
        _setup(own, geom, sigma)
        _build(own, fr, 0, geom, False, False)           # every other buffer of a build exists now
        full = [own.download_level(k, p, 0) for k in (0, MAX_BATCH - 1) for p in range(3)]
        own.set_option(OPT_L0_LAZY_GRAD, 2)
        for at in (0, MAX_BATCH - 1):                    # the first slot's plane; then, the first attempt having got none, the last slot's
            own.set_option(OPT_FAIL_ALLOC_AFTER, at)
            with pytest.raises(KltOutOfMemory):
                own.build_pyramids_batch(list(range(MAX_BATCH)), sync=True)
            own.set_option(OPT_FAIL_ALLOC_AFTER, -1)
        _build(own, fr, 2, geom, False, True)
        got = [own.download_level(k, p, 0) for k in (0, MAX_BATCH - 1) for p in range(3)]
        for a, b in zip(got, full):
            assert not first_difference(a, b)
    finally:
        own.close()


# ------------------------------------------------------------------------------------------------------------------------------- no GPU
def test_case_list_and_constants():
    """the constants above are the kernels' and the header's; every case takes its geometry under the host's rule at 32 frames and not with
    one frame fewer; widths, heights, both tap counts and both input types are all there for both geometries"""
    src = open(os.path.join(REPO, "pyfeaturetrack_amd", "csrc", "l0_plan.h")).read()
    assert re.search(r"L0S_TW = (\d+), L0S_SB = \d+, L0W_TW = (\d+)", src).groups() == ("64", "128")
    assert re.search(r"L0S_MIN_WGS = (\d+), L0W_MIN_WGS = (\d+)", src).groups() == (str(WORKGROUPS),) * 2
    assert re.search(r"shw = seg_of\(L0W_SB, (\d+)\), sh = seg_of\(L0S_SB, (\d+)\)", src).groups() == ("128", "160")
    hdr = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    assert re.search(r"#define\s+KLT_OPT_L0_LAZY_GRAD\s+(\d+)", hdr).group(1) == str(OPT_L0_LAZY_GRAD)
    assert re.search(r"#define\s+KLT_OPT_FAIL_ALLOC_AFTER\s+(\d+)", hdr).group(1) == str(OPT_FAIL_ALLOC_AFTER)
    for name, code in (("KLT_L0_STREAM", 5), ("KLT_L0_STREAM_NO_CENTRE", 6), ("KLT_L0_STREAM_WIDE", 7), ("KLT_L0_STREAM_WIDE_NO_CENTRE", 8)):
        assert re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1) == str(code)
    for geom, (_, strip, seg, _) in GEOMETRIES.items():
        mine = [c for c in CASES if c[0] == geom]
        assert [c[1] for c in mine[:3]] == [256, 257, 278]
        assert [c[2] for c in mine[3:]] == [seg - 1, seg + 1, seg + 17, 2 * seg + 3]
        for _, nc, nr, _ in mine:
            assert takes_geometry(geom, nc, nr) and not takes_geometry(geom, nc, nr, MAX_BATCH - 1), (geom, nc, nr)
            assert nc * nr * MAX_BATCH <= 36000000, (geom, nc, nr)
        if geom == "narrow":                             # (under value 1 the wide rule is not looked at; under 2 these would go wide)
            assert all(nc >= 2 * strip for _, nc, _, _ in mine)
        assert {c[3] for c in mine[:3]} == {0.1, 0.2} and {c[3] for c in mine[3:]} == {0.1, 0.2}
    assert TRACK_N * (MAX_BATCH // 2) == 2048


@pytest.mark.gpu
def test_tiled_launch_allocates_no_compact_plane():
    """a launch below the streaming bound (two 1024 x 1024 frames: the 32-row tile with the reduction) has no lean form: under option 1
    after a tracker launch with a lazy form has read both slots, and under option 2, the build is the full one, klt_level0_lean says 0,
    no compact plane is allocated (free device memory does not move: a plane would take 4 MB per slot) and the tracker's records stay"""
    from pyfeaturetrack_amd import synth
    from pyfeaturetrack_amd.backend import Context, FEAT_DTYPE
    RB32_HRED, n = 4, 2048
    f0, f1 = synth.synth_pair(1024, 1024, seed=9)
    rng = np.random.default_rng(9)
    fl = np.zeros(n, FEAT_DTYPE)
    fl["x"] = rng.uniform(130, 1024 - 130, n).astype(np.float32)
    fl["y"] = rng.uniform(130, 1024 - 130, n).astype(np.float32)
    own = Context(0)
    try:
        own.configure(make_tc(levels=3, ss=4))

        def step(lazy):
            own.set_option(OPT_L0_LAZY_GRAD, lazy)
            own.upload(0, f0)
            own.upload(1, f1)
            own.build_pyramids_batch([0, 1], sync=True)
            assert own.level0_path()[0] == RB32_HRED and not own.level0_lean()
            own.track_async(0, 1, 100, 200, n)
            own.sync()
            return own.featbuf_download(200, n).tobytes(), own.device_memory()[0]

        own.featbuf_upload(100, fl)
        first, free0 = step(1)                           # every buffer of a step exists now; both slots read by a launch with a lazy form
        for lazy in (1, 1, 2, 2):
            rec, free = step(lazy)
            assert rec == first
            assert free0 - free < (1 << 20), "option %d: free device memory fell by %d bytes" % (lazy, free0 - free)
    finally:
        own.close()
