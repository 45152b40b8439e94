"""What keeps tests/test_gpu_track_lazy_entry.py honest, without a GPU: the oracle runs the hand-placed list of that test on the same frames
and reports the Newton iterations of every feature at every level (want_iters; -1: level not visited).  The list was laid out so that
the four lane groups of a wavefront enter level 0 in every combination; here the oracle says that they do:

  - each of the 15 non-empty patterns of "reaches level 0 / does not" over records 4 k .. 4 k + 3 occurs in at least 4 wavefronts;
  - no pattern is filled only by lost input records: for every pattern with a group that stays behind, some wavefront of it has a
    LIVE feature that stops at a coarser level, and over the list both other reasons occur (small determinant in the flat block, out
    of bounds at the frame's edge);
  - at least 64 features do two or more iterations at level 0 (on the moving pairs), so footprints are requested inside the loop too;
  - on the unmoved pair the features that reach level 0 stop after one iteration: the entry phase's footprint is the only one."""
import numpy as np
import pytest

import test_gpu_track_lazy_entry as entry_mod
from helpers import params_from_tc

KLT_OOB = -4


@pytest.fixture(scope="module")
def frames6():
    return entry_mod.frames(3)


@pytest.mark.parametrize("name", list(entry_mod.PARAM_SETS))
def test_the_list_fills_every_pattern(frames6, name):
    from oracle import klt_oracle as ko
    p = params_from_tc(entry_mod.tc_of(name))
    fl = entry_mod.hand_list()
    live = fl["val"] >= 0
    ko.set_threads(8)
    try:
        runs = []
        for i in range(3):
            out = fl.copy()
            a0, a1 = frames6[2 * i].astype(np.float32), frames6[2 * i + 1].astype(np.float32)
            _, it = ko.track_features(p, ko.Pyramids(p, a0), ko.Pyramids(p, a1), out, want_iters=True)
            runs.append((out, it))
    finally:
        ko.set_threads(1)
    for i, (out, it) in enumerate(runs):
        reached = it[:, 0] >= 0
        assert not reached[~live].any()
        pat = entry_mod.wavefront_patterns(reached)
        count = np.bincount(pat, minlength=16)
        assert (count[1:] >= 4).all(), "%s, pair %d: wavefronts per pattern %r" % (name, i, count[1:])
        # a live feature that stays behind, in some wavefront of every pattern that has a group staying behind
        live_behind = (live & ~reached).reshape(-1, 4).any(axis=1)
        for m in range(1, 15):
            assert (live_behind & (pat == m)).any(), "%s, pair %d: pattern %d is filled by lost input records alone" % (name, i, m)
        # the three reasons.  (The final status word does not tell them apart: a feature that stops at a coarser level keeps that level's
        # coordinates, which lie inside the border, so its record says out of bounds either way.)  A live feature in the middle of the
        # large flat block has its windows inside every level: it can stop at the coarsest level without an iteration only on a small
        # determinant.  A live feature next to the frame's edge stops there because its window leaves the frame.
        coarsest = it[:, -1]
        bx, by, bs = entry_mod.BIG
        in_block = live & (np.abs(fl["x"] - (bx + bs / 2)) < 4) & (np.abs(fl["y"] - (by + bs / 2)) < 4)
        at_edge = live & ((np.minimum(fl["x"], fl["y"]) < 12) | (np.maximum(fl["x"], fl["y"]) > entry_mod.W - 13))
        assert in_block.sum() >= 16 and (coarsest[in_block] == 0).all() and not reached[in_block].any(), (in_block.sum(), coarsest[in_block])
        assert at_edge.sum() >= 16 and not reached[at_edge].any() and (out["val"][at_edge] == KLT_OOB).all()
        assert (~live).sum() >= 16
        assert reached[live & ~in_block & ~at_edge].mean() > 0.99, "the features placed inside textured ground should reach level 0"
    moving = np.concatenate([runs[0][1][:, 0], runs[2][1][:, 0]])
    assert (moving >= 2).sum() >= 64, "features with two or more level-0 iterations on the moving pairs: %d" % (moving >= 2).sum()
    still = runs[1][1][:, 0]
    assert (still[still >= 0] <= 1).mean() > 0.95, "the unmoved pair should stop after one level-0 iteration"
