"""The plain 7x7 quad tracker with level-0 gradients on demand (track_kernel_quad<..., 1 + LAZY_WAVES>, KLT_OPT_L0_LAZY_GRAD): on slots
whose level 0 is the compact smoothed image of a lean build it must give the records of the same call on full slots byte for byte, and
the CPU oracle's positions and status words without a tolerance.

All cases work on ONE batch of 32 frames of 1024 x 1024 (the smallest square batch the production rule sends to the wide streaming
kernel: 8 strips x 8 segments x 32 frames = 2048 workgroups), built once full (option 0) and once lean (option 2) per parameter set;
the full build's records are computed once per parameter set and shared.  That the lazy kernel ran -- and not the fallback that makes the
records first -- is asserted through the context's launch counters: no gradient launch between the build and the download.

Part one: klt_track_async (one pair, 2048 features) and klt_track_batch_async (16 pairs of 2048) with lists the selector placed; pairs 0,
7 and 15 against the oracle.

Part two: a hand-placed list of 2048 records on three pairs (moved by (1.3, -0.8); not moved at all; moved by (9.7, -6.3)) under four
parameter sets.  What it holds: features whose level-0 footprint touches row 0, column 0, the last row and the last column (with two or
more levels such a feature leaves the image at a coarser level first, in every implementation: the reflect map of the patch is what
keeps the lanes of finished features inside the plane), features a few pixels further in whose 14 x 14 patch ends at the frame's
edge, lost input records, templates out of bounds, features on a flat patch (small determinant), features on the unmoved pair (they stay
in one integer corner: the footprint is reused), a step factor of 2.5 with four iterations (steps of more than a pixel, the iteration
limit), the residue test on and off.  And a launch that mixes a lean slot with a full one, which must give the same records through the
fallback."""
import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from pyramid_expected import MAX_BATCH, OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM

OPT_L0_LAZY_GRAD = 22
W = H = 1024
N = 2048
NPAIRS = MAX_BATCH // 2
STREAM_WIDE_NO_CENTRE = 8
FLAT = (600, 300, 64)                                # x0, y0, side of the constant block in every frame
EXTRA_SLOT = 40                                      # a frame built on its own (the tiled kernel: always full)
IN0, OUT0 = 100, 200


def _frames():
    """32 frames of one periodic texture: pair i = slots (2 i, 2 i + 1).  Pair 1 does not move, pair 2 moves by (9.7, -6.3), every other
    pair by (1.3, -0.8); each pair starts from its own phase.  A constant block sits at the same place in every frame."""
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(W, H, 5)
    out = []
    for i in range(NPAIRS):
        dx, dy = {1: (0.0, 0.0), 2: (9.7, -6.3)}.get(i, (1.3, -0.8))
        for k in range(2):
            f = synth.shift_frame(base, 7.0 * i + k * dx, -3.0 * i + k * dy)
            x0, y0, s = FLAT
            f[y0:y0 + s, x0:x0 + s] = 128
            out.append(f)
    return out


PARAM_SETS = {
    "default": dict(),
    "residue": dict(max_residue=10.0),
    "tight-residue": dict(max_residue=0.1),
    "big-steps": dict(step_factor=2.5, max_iterations=4),
}


def _tc(name):
    return make_tc(levels=3, ss=4, **PARAM_SETS[name])


def _hand_list():
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    rng = np.random.default_rng([2048, 9])
    fl = np.zeros(N, FEAT_DTYPE)
    fl["x"] = rng.uniform(130, W - 130, N).astype(np.float32)      # fillers: live features anywhere inside the border
    fl["y"] = rng.uniform(130, H - 130, N).astype(np.float32)
    hand = []
    for e in (3.0, 3.5, 3.999, 4.0, 6.5, 7.0, 11.9, 12.0, 15.5, 16.0, 19.99, 27.5):     # distance of the window centre from an edge
        hand += [(e, 500.25), (500.25, e), (W - 1 - e, 500.75), (500.75, H - 1 - e), (e, e), (W - 1 - e, H - 1 - e), (e, H - 1 - e), (W - 1 - e, e)]
    hand += [(-5.0, 400.0), (400.0, -0.5), (W + 3.0, 400.0), (400.0, H + 0.25), (2.5, 2.5), (W - 2.0, H - 2.0)]      # templates out of bounds
    x0, y0, s = FLAT
    hand += [(x0 + 8.0 + 6 * i, y0 + 8.5 + 6 * j) for i in range(8) for j in range(8)]                                # flat: small determinant
    hand += [(x0 - 2.0 + 0.5 * i, y0 + 30.0) for i in range(12)] + [(x0 + 30.0, y0 + s - 4.0 + 0.5 * i) for i in range(12)]   # its edges
    hand += [(200.0 + 0.125 * i, 700.0 + 0.0625 * i) for i in range(32)]                                               # a run of sub-pixel phases
    for i, (x, y) in enumerate(hand):
        fl["x"][4 * i], fl["y"][4 * i] = x, y                      # spread over the wavefronts: every fourth record
    lost = np.arange(1, N, 37)
    fl["val"][lost] = -1 - (np.arange(lost.size) % 5)               # lost input records, every status
    fl["x"][lost[::2]] = -1.0
    fl["y"][lost[::2]] = -1.0
    assert 4 * len(hand) <= N
    return fl


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.set_option(OPT_L0_LAZY_GRAD, 1)
    c.close()


@pytest.fixture(scope="module")
def frames32():
    return _frames()


def _build(ctx, fr, name, lazy):
    ctx.configure(_tc(name))
    ctx.set_option(OPT_FUSED_KERNELS, 1)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, 2)
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)
    for k, f in enumerate(fr):
        ctx.upload(k, f)
    ctx.build_pyramids_batch(list(range(len(fr))), sync=True)
    assert ctx.level0_path()[0] == STREAM_WIDE_NO_CENTRE and ctx.level0_lean() == (lazy == 2)
    ctx.upload(EXTRA_SLOT, fr[1])
    ctx.build_pyramids_batch([EXTRA_SLOT], sync=True)
    assert not ctx.level0_lean()
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)


def _launches(ctx):
    return {t["name"]: t["launches"] for t in ctx.timing_read()}


def _run(ctx, calls, lazy_expected):
    """the tracker calls under the launch counters: (records per call, launches by family)"""
    ctx.timing_enable(True)
    try:
        outs = []
        for kind, pairs in calls:
            if kind == "single":
                (s1, s2, fi, fo), = pairs
                ctx.track_async(s1, s2, fi, fo, N)
            else:
                ctx.track_batch_async(pairs, N)
            ctx.sync()
            outs.append([ctx.featbuf_download(p[3], N) for p in pairs])
        seen = _launches(ctx)
    finally:
        ctx.timing_enable(False)
    assert seen.get("track", 0) == len(calls), seen
    if lazy_expected:
        assert seen.get("gradients", 0) == 0, "level-0 records were made for a launch that has a lazy form: %r" % seen
    return outs


def _oracle(name, f0, f1, fl):
    from benchlib.common import oracle_track
    from oracle import klt_oracle as ko
    return oracle_track(ko, params_from_tc(_tc(name)), f0, f1, fl, threads=8)


def _same_as_oracle(got, want, what):
    assert np.array_equal(got["val"], want["val"]), "%s: status words differ from the oracle's at %r" % (what, np.flatnonzero(got["val"] != want["val"])[:8])
    for k in ("x", "y"):
        assert np.array_equal(got[k], want[k].astype(np.float32)), "%s: %s differs from the oracle's at %r" % (what, k, np.flatnonzero(got[k] != want[k])[:8])


# ---------------------------------------------------------------------------------------------------------------------------- part one
@pytest.mark.gpu
def test_selected_lists_single_and_batched(ctx, frames32):
    fr = frames32
    _build(ctx, fr, "residue", 0)
    lists = []
    for i in range(NPAIRS):
        fl, placed = ctx.select(2 * i, N, use_pyramid=True)
        assert placed == N
        lists.append(fl)
        ctx.featbuf_upload(IN0 + i, fl)
    calls = [("single", [(0, 1, IN0, OUT0)]), ("batch", [(2 * i, 2 * i + 1, IN0 + i, OUT0 + i) for i in range(NPAIRS)]),
             ("single", [(6, 7, IN0 + 3, OUT0 + 3)])]
    full = _run(ctx, calls, False)
    _build(ctx, fr, "residue", 2)
    lean = _run(ctx, calls, True)
    for c, (a, b) in enumerate(zip(full, lean)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.tobytes() == y.tobytes(), "call %d, pair %d: the records on lean slots differ from those on full ones" % (c, i)
    assert (lean[1][0]["val"] == 0).sum() > N // 2, "pair 0 should mostly be tracked"
    for i in (0, 7, 15):
        _same_as_oracle(lean[1][i], _oracle("residue", fr[2 * i], fr[2 * i + 1], lists[i]), "batched launch, pair %d" % i)
    _same_as_oracle(lean[0][0], _oracle("residue", fr[0], fr[1], lists[0]), "single launch")


# ---------------------------------------------------------------------------------------------------------------------------- part two
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_hand_placed_list(ctx, frames32, name):
    fr = frames32
    fl = _hand_list()
    calls = [("single", [(0, 1, IN0, OUT0)]), ("single", [(2, 3, IN0, OUT0 + 1)]), ("single", [(4, 5, IN0, OUT0 + 2)]),
             ("batch", [(0, 1, IN0, OUT0 + 3), (2, 3, IN0, OUT0 + 4), (4, 5, IN0, OUT0 + 5)])]
    _build(ctx, fr, name, 0)
    ctx.featbuf_upload(IN0, fl)
    full = _run(ctx, calls, False)
    _build(ctx, fr, name, 2)
    lean = _run(ctx, calls, True)
    for c, (a, b) in enumerate(zip(full, lean)):
        for i, (x, y) in enumerate(zip(a, b)):
            assert x.tobytes() == y.tobytes(), "%s, call %d, pair %d: the records on lean slots differ from those on full ones" % (name, c, i)
    for i in range(3):
        want = _oracle(name, fr[2 * i], fr[2 * i + 1], fl)
        _same_as_oracle(lean[i][0], want, "%s, pair %d" % (name, i))
        _same_as_oracle(lean[3][i], want, "%s, pair %d of the batched launch" % (name, i))
    live = fl["val"] >= 0
    vals = np.concatenate([lean[i][0]["val"][live] for i in range(3)])
    assert np.array_equal(lean[0][0][~live], fl[~live]), "lost input records must pass through unchanged"
    # the cases the list was written for do occur: tracked, out of bounds, small determinant; and with them switched on, the iteration
    # limit and the residue
    assert (vals == 0).sum() > N // 2 and (vals == -4).sum() >= 24 and (vals == -2).sum() >= 16, np.unique(vals, return_counts=True)
    if name == "big-steps":
        assert (vals == -3).sum() >= 16, np.unique(vals, return_counts=True)
    if name == "tight-residue":
        assert (vals == -5).sum() >= 16, np.unique(vals, return_counts=True)
    if name == "default":
        assert (vals == -5).sum() == 0
    iters0 = lean[1][0]["aux"][live & (lean[1][0]["val"] == 0)] & 15
    assert (iters0 >= 2).all(), "aux holds the iterations of level 0 + 1"

    # a launch that mixes a lean slot with a full one: the records of the full pair, through the fallback
    mixed = _run(ctx, [("single", [(0, EXTRA_SLOT, IN0, OUT0 + 6)])], False)
    assert mixed[0][0].tobytes() == full[0][0].tobytes(), "%s: lean slot 0 with full slot %d" % (name, EXTRA_SLOT)
    # ... after which slot 0 holds both forms, slot 1 still the compact image alone: lazy again, same records
    again = _run(ctx, [("single", [(0, 1, IN0, OUT0 + 7)])], True)
    assert again[0][0].tobytes() == full[0][0].tobytes()


# ------------------------------------------------------------------------------------------------ the resident-pair flow of the headline
@pytest.mark.gpu
def test_resident_pairs_go_lean_from_the_second_step():
    """bench.py's cfg-2 in small, under the default option (adaptive): eight resident 1080p pairs built in one batch, a selection on the
    first frame of every pair, then steps of build + batched tracker.  The step after the selection is built full, every later one lean
    (klt_level0_lean), and every step gives the records of the same step with the option switched off."""
    from benchlib.common import NFEAT, cfg2_context
    from pyfeaturetrack_amd import synth
    from pyfeaturetrack_amd.backend import Context
    B = 8
    pairs = [synth.synth_pair(1920, 1080, seed=s + 1) for s in range(B)]
    slots = list(range(2 * B))
    records = {}
    for lazy in (0, 1):
        cx = Context(0)
        try:
            cx.set_params(params_from_tc(cfg2_context()))
            cx.set_option(OPT_L0_LAZY_GRAD, lazy)
            for i, (f0, f1) in enumerate(pairs):
                cx.upload(2 * i, f0)
                cx.upload(2 * i + 1, f1)
            cx.build_pyramids_batch(slots)
            assert not cx.level0_lean()                  # a slot's first build is full
            for i in range(B):
                fl, placed = cx.select(2 * i, NFEAT, use_pyramid=True)
                assert placed == NFEAT
                cx.featbuf_upload(IN0 + i, fl)
            lean, outs = [], []
            for step in range(4):
                cx.build_pyramids_batch(slots)
                lean.append(cx.level0_lean())
                cx.track_batch_async([(2 * i, 2 * i + 1, IN0 + i, OUT0 + i) for i in range(B)], NFEAT)
                cx.sync()
                outs.append([cx.featbuf_download(OUT0 + i, NFEAT).tobytes() for i in range(B)])
            assert lean == ([False, True, True, True] if lazy else [False] * 4), lean
            records[lazy] = outs
        finally:
            cx.close()
    for step in range(4):
        assert records[1][step] == records[0][0], "step %d: the records differ from those of full builds" % step
        assert records[0][step] == records[0][0]
