"""KLT_OPT_TRACK_LAZY_FORM: the fused level-0 entry phase of the lazy 7x7 quad tracker (lazy_records_entry: the gradients of the template's
footprint and of the first search footprint made in one phase) against the form that makes them one after the other, against the
tracker on full records, and against the CPU oracle -- byte for byte, no tolerance.

The batch has the shape of test_gpu_track_lazy.py's: 32 frames of 1024 x 1024 (the smallest batch the level-0 plan sends to a lean
streaming launch; the same texture and motions, with a second, larger constant block), built once full and once lean per parameter
set, at 3 levels / subsampling 4 and at 2 levels / subsampling 4.  Pair 0 moves by (1.3,
-0.8), pair 1 not at all (every feature stays in one integer corner: the footprint of the entry phase is the only one), pair 2 by
(9.7, -6.3); "big-steps" (step factor 2.5, four iterations) makes features change corner inside the Newton loop, where both forms
recompute a footprint alone.

The list is placed by hand so that the four features of a wavefront (records 4 k .. 4 k + 3 with KLT_OPT_TRACK_XCD_ORDER off) take part
in the entry phase in every combination: each of the 15 non-empty patterns of "reaches level 0 / does not" over the four lane groups
is laid out in eight wavefronts, and a group that does not reach level 0 fails for one of three reasons in turn -- a lost input
record, a feature in the middle of the frames' large flat block (352 pixels wide, 22 at level 2: flat under the coarsest level's window,
its gradient taps and the pyramid's smoothing, so the determinant is small there), a feature a few pixels from the frame's edge (out
of bounds at the coarsest level).  tests/test_track_lazy_entry_rule.py holds the list against the oracle without a GPU:
the patterns do occur, for every reason, and enough features iterate at level 0.  The same list runs with the XCD order on, where the
wavefronts are made of other records."""
import numpy as np
import pytest

import test_gpu_track_lazy as lazy_mod
from helpers import make_tc, params_from_tc
from pyramid_expected import OPT_FUSED_HREDUCE, OPT_FUSED_KERNELS, OPT_L0_STREAM

OPT_XCD_ORDER, OPT_L0_LAZY_GRAD, OPT_TRACK_LAZY_FORM = 13, 22, 24
W, H, N = lazy_mod.W, lazy_mod.H, lazy_mod.N
IN0, OUT0 = lazy_mod.IN0, lazy_mod.OUT0
REPS = 8                                             # wavefronts laid out per pattern
BIG = (120, 540, 352)                                # x0, y0, side of the large constant block in every frame


def frames(npairs=lazy_mod.NPAIRS):
    """test_gpu_track_lazy._frames with the large block added: pair i = frames (2 i, 2 i + 1); pair 1 does not move, pair 2 moves by (9.7,
    -6.3), every other pair by (1.3, -0.8)"""
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(W, H, 5)
    out = []
    for i in range(npairs):
        dx, dy = {1: (0.0, 0.0), 2: (9.7, -6.3)}.get(i, (1.3, -0.8))
        for k in range(2):
            f = synth.shift_frame(base, 7.0 * i + k * dx, -3.0 * i + k * dy)
            for x0, y0, s in (lazy_mod.FLAT, BIG):
                f[y0:y0 + s, x0:x0 + s] = 128
            out.append(f)
    return out


PARAM_SETS = {
    "3-levels": dict(levels=3, ss=4),
    "2-levels": dict(levels=2, ss=4),
    "big-steps": dict(levels=3, ss=4, step_factor=2.5, max_iterations=4),
}


def tc_of(name):
    kw = dict(PARAM_SETS[name])
    return make_tc(levels=kw.pop("levels"), ss=kw.pop("ss"), **kw)


def hand_list():
    """2048 records; wavefront 8 (m - 1) + rep holds pattern m (bit i: lane group i reaches level 0), the rest are live features anywhere"""
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    rng = np.random.default_rng([2048, 49])
    fl = np.zeros(N, FEAT_DTYPE)
    x0, y0, side = BIG

    def good(k):
        # inside the border, and so far from the flat blocks that no level's window sees one
        while True:
            x, y = rng.uniform(130, W - 130), rng.uniform(130, H - 130)
            if not any(bx - 140 < x < bx + bs + 140 and by - 140 < y < by + bs + 140 for bx, by, bs in (lazy_mod.FLAT, BIG)):
                return np.float32(x), np.float32(y)

    for k in range(N):
        fl["x"][k], fl["y"][k] = good(k)
    for m in range(1, 16):
        for rep in range(REPS):
            w = REPS * (m - 1) + rep
            for i in range(4):
                if m >> i & 1:
                    continue
                k, cause = 4 * w + i, (rep + i) % 3
                if cause == 0:                           # a lost input record
                    fl["val"][k] = -1 - (w + i) % 5
                    if rep & 1:
                        fl["x"][k] = fl["y"][k] = -1.0
                elif cause == 1:                         # the middle of the large flat block
                    fl["x"][k] = x0 + side / 2 + rng.uniform(-3, 3)
                    fl["y"][k] = y0 + side / 2 + rng.uniform(-3, 3)
                else:                                    # 5 .. 11 pixels from an edge: the coarsest level's window leaves the frame
                    e, t = rng.uniform(5, 11), rng.uniform(200, W - 200)
                    fl["x"][k], fl["y"][k] = [(e, t), (t, e), (W - 1 - e, t), (t, H - 1 - e)][(w + i) % 4]
    return fl


def wavefront_patterns(reached):
    """reached[k]: record k reaches level 0 -> the pattern (4 bits) of every wavefront of the list in list order"""
    r = np.asarray(reached, bool).reshape(-1, 4)
    return r[:, 0] * 1 + r[:, 1] * 2 + r[:, 2] * 4 + r[:, 3] * 8


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames32():
    return frames()


def _build(ctx, fr, name, lazy):
    ctx.configure(tc_of(name))
    ctx.set_option(OPT_FUSED_KERNELS, 1)
    ctx.set_option(OPT_FUSED_HREDUCE, 1)
    ctx.set_option(OPT_L0_STREAM, 2)
    ctx.set_option(OPT_L0_LAZY_GRAD, lazy)
    for k, f in enumerate(fr):
        ctx.upload(k, f)
    ctx.build_pyramids_batch(list(range(len(fr))), sync=True)
    assert ctx.level0_lean() == (lazy == 2), "KLT_OPT_L0_LAZY_GRAD %d: klt_level0_lean says %r" % (lazy, ctx.level0_lean())


SINGLES = [("single", [(2 * i, 2 * i + 1, IN0, OUT0 + i)]) for i in range(3)]
BATCH = [("batch", [(2 * i, 2 * i + 1, IN0, OUT0 + 3 + i) for i in range(3)])]


def _records(ctx, lazy_expected):
    """the list on pairs 0, 1, 2, each alone and the three in one batched launch, XCD order off and on: [order][call][pair] -> bytes"""
    out = []
    for order in (0, 1):
        ctx.set_option(OPT_XCD_ORDER, order)
        out.append(lazy_mod._run(ctx, SINGLES + BATCH, lazy_expected))
    ctx.set_option(OPT_XCD_ORDER, 1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_entry_forms_full_records_and_oracle(ctx, frames32, name):
    fr, fl = frames32, hand_list()
    _build(ctx, fr, name, 0)
    ctx.featbuf_upload(IN0, fl)
    full = _records(ctx, False)
    _build(ctx, fr, name, 2)
    forms = {}
    for form in (0, 1):
        ctx.set_option(OPT_TRACK_LAZY_FORM, form)
        forms[form] = _records(ctx, True)
    ctx.set_option(OPT_TRACK_LAZY_FORM, 1)
    for form in (0, 1):
        for order in (0, 1):
            for c, (a, b) in enumerate(zip(full[order], forms[form][order])):
                for i, (x, y) in enumerate(zip(a, b)):
                    assert x.tobytes() == y.tobytes(), "%s, form %d, XCD order %d, call %d, pair %d: the records on lean slots differ from " \
                        "those on full ones at %r" % (name, form, order, c, i, np.flatnonzero(x != y)[:8])
    from benchlib.common import oracle_track
    from oracle import klt_oracle as ko
    for i in range(3):
        want = oracle_track(ko, params_from_tc(tc_of(name)), fr[2 * i], fr[2 * i + 1], fl, threads=8)
        for order in (0, 1):
            lazy_mod._same_as_oracle(forms[1][order][i][0], want, "%s, form 1, XCD order %d, pair %d" % (name, order, i))
            lazy_mod._same_as_oracle(forms[1][order][3][i], want, "%s, form 1, XCD order %d, pair %d of the batched launch" % (name, order, i))
    live = fl["val"] >= 0
    assert np.array_equal(forms[1][0][0][0][~live], fl[~live]), "lost input records must pass through unchanged"
