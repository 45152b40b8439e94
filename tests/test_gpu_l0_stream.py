"""KLT_OPT_L0_STREAM: the streaming level-0 kernel (a workgroup walks a column strip down in bands) and the tiled kernel build the
same pyramids bit for bit -- level-0 image, both gradients and levels 1 and 2, u8 and f32 frames, 5- and 9-tap smoothing, frame
sizes that are not multiples of the strip, the band or the segment, and batches of 1 to 16 frames (the launches below the
streaming kernel's grid bound take the tiled kernel both ways: 640 x 480 x 16, and 1921 x 1083 in batches of 1, 2 and 8).  Which
kernel each build launched is asserted through klt_level0_path, so that a retuned bound cannot turn a case into "tiled both ways"
unnoticed.  tests/test_gpu_l0_edges.py sweeps the strip, band and segment remainders with batches of small frames."""
import os
import re

import numpy as np
import pytest

from helpers import make_tc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = 3


def _option():
    hdr = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    return int(re.search(r"#define\s+KLT_OPT_L0_STREAM\s+(\d+)", hdr).group(1))


OPT_L0_STREAM = _option()


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _frames(shape, n, f32, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    out = []
    for k in range(n):
        smooth = 128 + 90 * np.sin(xx / (7.0 + k) + 0.3 * k) * np.cos(yy / (11.0 + k))
        img = np.clip(smooth + rng.normal(0, 25, shape), 0, 255)
        out.append(img.astype(np.float32) if f32 else img.astype(np.uint8))
    return out


STREAM_CODES, TILED_CODES = (5, 6), (2, 3, 4)        # klt_level0_path: KLT_L0_STREAM*, KLT_L0_RB16 / RB32 / RB32_HRED


def _build(ctx, frames, stream, streams=True):
    """`streams`: the launch is large enough for the streaming kernel (asserted through klt_level0_path both ways)"""
    ctx.set_option(OPT_L0_STREAM, stream)
    try:
        for i, f in enumerate(frames):
            ctx.upload(i, f)
        ctx.build_pyramids_batch(list(range(len(frames))), sync=True)
        code = ctx.level0_path()[0]
        assert code in (STREAM_CODES if stream and streams else TILED_CODES), "option %d, streams %d: level-0 kernel code %d" % (stream, streams, code)
        return [[ctx.download_level(i, p, l) for l in range(LEVELS) for p in range(3)] for i in range(len(frames))]
    finally:
        ctx.set_option(OPT_L0_STREAM, 1)


def _check(ctx, frames, tc, what, streams=True):
    ctx.configure(tc)
    on, off = _build(ctx, frames, 1, streams), _build(ctx, frames, 0, streams)
    names = ["%s level %d" % (w, l) for l in range(LEVELS) for w in ("img", "gx", "gy")]
    for i, (a_planes, b_planes) in enumerate(zip(on, off)):
        for name, a, b in zip(names, a_planes, b_planes):
            assert a.shape == b.shape, "%s, frame %d, %s: shape %s vs %s" % (what, i, name, a.shape, b.shape)
            bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
            if bad.size:
                j = bad[0]
                raise AssertionError("%s, frame %d, %s: %d of %d differ; first at flat index %d: %r (stream) vs %r (tiled)" %
                                     (what, i, name, bad.size, a.size, j, a.ravel()[j], b.ravel()[j]))


# (rows, cols), frames per launch.  The streaming kernel runs where its grid (64-column strips x 160-row segments x frames) has
# >= 2048 workgroups: 1280 x 1024 x 16 and 10240 x 128 x 16 are exactly at that bound, 640 x 480 x 16 stays below it (tiled both ways)
CASES = [((1080, 1920), 16), ((1083, 1921), 16), ((480, 640), 16), ((2160, 3840), 3), ((1280, 1024), 16), ((10240, 128), 16)]


@pytest.mark.parametrize("shape,n", CASES)
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("sigma_fact", [0.1, 0.2])      # 5- and 9-tap smoothing at the default window
def test_stream_equals_tiled_shapes(ctx, shape, n, f32, sigma_fact):
    tc = make_tc(levels=LEVELS, ss=4, smooth_sigma_fact=sigma_fact)
    _check(ctx, _frames(shape, n, f32, shape[0] + shape[1]), tc, "%dx%d x%d %s sigma %.1f" % (shape[1], shape[0], n, "f32" if f32 else "u8", sigma_fact),
           streams=shape != (480, 640))


@pytest.mark.parametrize("batch", [1, 2, 8, 16])
@pytest.mark.parametrize("f32", [False, True])
def test_stream_equals_tiled_batches(ctx, batch, f32):
    tc = make_tc(levels=LEVELS, ss=4)
    # 31 strips x 7 segments per frame: only the batch of 16 fills the grid bound of 2048 workgroups, batches of 1, 2 and 8 (1736 workgroups)
    # take the tiled kernel both ways
    _check(ctx, _frames((1083, 1921), batch, f32, batch), tc, "1921x1083 x%d %s" % (batch, "f32" if f32 else "u8"), streams=31 * 7 * batch >= 2048)


@pytest.mark.parametrize("sigma_fact", [0.1, 0.2])
def test_stream_equals_tiled_negative_and_signed_zero_f32(ctx, sigma_fact):
    """f32 frames may hold negative values, -0.0 and infinities: the derivative passes keep their centre multiply there (an
    infinite centre times the +0.0 centre tap is NaN; a -0 / +0 step inside a constant region leaves only the centre product's +0)"""
    frames = _frames((1080, 1920), 16, True, 7)
    for k, f in enumerate(frames):
        f -= 128.0
        f[:, 200 + 64 * k:260 + 64 * k] = -0.0
        f[500:540, :] = np.float32(-0.0)
        f[700:702, 300:900] = 0.0
        f[100:300, 1000:1200] = np.float32(-0.0)
        f[100:300, 1100:1200] = np.float32(0.0)
        f[400 + 13 * k, 1500 + 7 * k] = np.float32(np.inf)
        f[900, 640 + k] = np.float32(-np.inf)
    tc = make_tc(levels=LEVELS, ss=4, smooth_sigma_fact=sigma_fact)
    _check(ctx, frames, tc, "signed f32 sigma %.1f" % sigma_fact)
