"""A slot's pyramid levels are planes of 12-byte pixel records (image, gradx, grady side by side).  Every plane of every level, as the
ABI downloads it, is bit-identical to the oracle's (and to the goldens at cfg-1): u8 and f32 frames, cfg-1 and cfg-2 sizes, 5- and
9-tap smoothing, and tap sets the specialised kernels do not take.  Selection from the pyramid and tracking on the records then give the
oracle's features."""
import numpy as np
import pytest

from helpers import make_tc, params_from_tc

pytestmark = pytest.mark.gpu
PLANES = ("img", "gx", "gy")


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ko():
    from oracle import klt_oracle
    return klt_oracle


def _same(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    if bad.size:
        i = bad[0]
        raise AssertionError("%s: %d of %d differ; first at flat index %d: %r vs %r" % (what, bad.size, a.size, i, a.ravel()[i], b.ravel()[i]))


def _frames(shape, n, f32):
    """n frames of one scene, each shifted a little further (frame k + 1 tracks from frame k)"""
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(shape[1], shape[0], 5)
    out = []
    for k in range(n):
        f = synth.shift_frame(base, 0.7 * k, -0.4 * k)
        out.append(f.astype(np.float32) + np.float32(0.25) if f32 else f)
    return out


def _check_levels(ctx, ko, p, frames, slots, levels, what):
    pyr = {}
    for s in slots:
        P = ko.Pyramids(p, frames[s].astype(np.float32))
        pyr[s] = P
        for l in range(levels):
            for pi, w in enumerate(PLANES):
                _same(ctx.download_level(s, pi, l), P.level(w, l), "%s, frame %d, %s level %d" % (what, s, w, l))
    return pyr


def _select_and_track(ctx, ko, p, frames, pyr, what, nfeat):
    fl, _ = ctx.select(0, nfeat, use_pyramid=True)
    ofl = ko.select_good_features(p, frames[0].astype(np.float32), nfeat)
    for k in ("x", "y", "val"):
        assert np.array_equal(fl[k], ofl[k]), "%s: selection %s" % (what, k)
    out, _ = ctx.track(0, 1, fl)
    ko.track_features(p, pyr[0], pyr[1], ofl)
    for k in ("x", "y", "val"):
        assert np.array_equal(out[k], ofl[k]), "%s: tracking %s" % (what, k)


# (rows, cols), frames per build: cfg-1 (two frames: the tiled level-0 kernel, level 1 reduced from a compact copy of level 0) and
# cfg-2 (sixteen 1080p frames: the streaming level-0 kernel with the fused first reduction)
@pytest.mark.parametrize("shape,n", [((240, 320), 2), ((1080, 1920), 16)])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("sigma_fact", [0.1, 0.2])      # 5- and 9-tap smoothing at the default window
def test_record_planes_equal_the_oracle(ctx, ko, shape, n, f32, sigma_fact):
    levels = 3 if shape[0] > 500 else 2
    tc = make_tc(levels=levels, ss=4, smooth_sigma_fact=sigma_fact, max_residue=10.0)
    p = params_from_tc(tc)
    ctx.configure(tc)
    frames = _frames(shape, n, f32)
    for i, f in enumerate(frames):
        ctx.upload(i, f)
    ctx.build_pyramids_batch(list(range(n)), sync=True)
    what = "%dx%d x%d %s sigma %.1f" % (shape[1], shape[0], n, "f32" if f32 else "u8", sigma_fact)
    pyr = _check_levels(ctx, ko, p, frames, sorted({0, 1, n // 2, n - 1}), levels, what)
    _select_and_track(ctx, ko, p, frames, pyr, what, 300)


def test_record_planes_equal_the_goldens(ctx, cfg1, img0, img1):
    """the cfg-1 goldens, through the batched build (u8, u8 and f32 frames: two launch groups) and the generic two-pass kernels"""
    ctx.configure(make_tc())
    ctx.upload(0, img0)
    ctx.upload(1, img1)
    ctx.upload(2, img1.astype(np.float32))
    ctx.build_pyramids_batch([0, 1, 2], sync=True)
    for slot, name in ((0, "p0"), (1, "p1"), (2, "p1")):
        for l in range(2):
            for pi, w in enumerate(PLANES):
                _same(ctx.download_level(slot, pi, l), cfg1["%s_%s_%d" % (name, w, l)], "batched slot %d %s %d" % (slot, w, l))
    try:
        ctx.set_option(1, 0)                                    # KLT_OPT_FUSED_KERNELS off: generic kernels + record packing
        ctx.build_pyramids_batch([0, 1, 2], sync=True)
        for slot, name in ((0, "p0"), (1, "p1"), (2, "p1")):
            for l in range(2):
                for pi, w in enumerate(PLANES):
                    _same(ctx.download_level(slot, pi, l), cfg1["%s_%s_%d" % (name, w, l)], "generic slot %d %s %d" % (slot, w, l))
    finally:
        ctx.set_option(1, 1)


# tap sets the compile-time specialisations do not take: runtime-sized gradient kernels, generic reductions
@pytest.mark.parametrize("attrs,levels,ss", [({"grad_sigma": 1.5}, 2, 4), ({"pyramid_sigma_fact": 0.6}, 3, 4),
                                             ({"smooth_sigma_fact": 0.3}, 2, 2)])
@pytest.mark.parametrize("f32", [False, True])
def test_record_planes_non_specialised_taps(ctx, ko, attrs, levels, ss, f32):
    tc = make_tc(levels=levels, ss=ss, max_residue=20.0, **attrs)
    p = params_from_tc(tc)
    ctx.configure(tc)
    frames = _frames((220, 300), 2, f32)
    for i, f in enumerate(frames):
        ctx.upload(i, f)
    ctx.build_pyramids_batch([0, 1], sync=True)
    what = "%s %s" % (attrs, "f32" if f32 else "u8")
    pyr = _check_levels(ctx, ko, p, frames, [0, 1], levels, what)
    _select_and_track(ctx, ko, p, frames, pyr, what, 30)


def test_selection_scratch_records(ctx, ko, img0):
    """the selection's own planes (use_pyramid=0) are pixel records as well: their downloads are the oracle's smoothed image and
    gradients"""
    tc = make_tc()
    ctx.configure(tc)
    ctx.upload(0, img0)
    ctx.select(0, 100, use_pyramid=False)
    P = ko.Pyramids(params_from_tc(tc), img0.astype(np.float32))
    for pi, w in enumerate(PLANES):
        _same(ctx.select_intermediate(pi), P.level(w, 0), "selection %s" % w)
