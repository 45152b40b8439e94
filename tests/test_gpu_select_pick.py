"""The second half of selection at the edges of its tiles, cuts and loops (the tables of tests/select_pick_expected.py): the top-K cut, the
parallel minimum-distance passes with their ranking and placement, the greedy walk and the live-feature squares, on given scores
(klt_set_score_override) under KLT_OPT_SELECT_PARALLEL_NMS 1 and 0.  Every case compares x, y and val of every slot and the placed count
with the CPU oracle (ko.sorted_candidates + ko.enforce_min_distance; klt_min_distance_walk with oracle/min_distance_walk.py) bit for bit,
and asserts through klt_select_pick_path that the code it was written for is the code that ran."""
import pytest

from select_pick_expected import CUT, DRAW_SEEDS, PASSES, REPLACE, WALK, case_id, draw_entry, run_pick_trial, run_walk_trial

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _run(ctx, entry):
    bad = run_pick_trial(ctx, entry)
    assert bad is None, "%s\n%r" % (bad, entry)


@pytest.mark.parametrize("entry", PASSES, ids=case_id)
def test_passes_entry(ctx, entry):
    """SELECTING_ALL: every exclusion radius at which mis_round_tile, its staging loops, the dynamic-LDS attribute or the choice of walk
    changes, on a lattice without and with an interior tile; tile counts around the 8 XCDs; ties, plateaus, ramps and checkerboards; tiles
    filled to exactly their capacity; scores at the threshold and at the largest int; ranking by counting against sorting at a bound of
    98304; accepted counts around the 96 chunks of mis_rank_kernel against list lengths around them; more than 4096 tiles"""
    _run(ctx, entry)


@pytest.mark.parametrize("entry", REPLACE, ids=case_id)
def test_replace_entry(ctx, entry):
    """REPLACING_SOME: live features at the fractional parts .0 / .49 / .5 / .51, in the first and last candidate column and row, near
    the frame edge, in the border margin, with overlapping squares, with and without skipped pixels; 0, 1 and all slots lost; lists either
    side of 256, 4096 and 8192 slots with lost slots at their edges and at every multiple of 256"""
    _run(ctx, entry)


@pytest.mark.parametrize("entry", CUT, ids=case_id)
def test_cut_entry(ctx, entry):
    """more than 262144 candidates: the prefilter planned and not, targets either side of half the candidates, fewer valid keys than the
    target, one bin, two bins, cuts that hold and cuts whose candidates run out (the repeat with every candidate, asserted), replacement
    behind the cut, and the frame whose histogram sample sees nothing of what the cut drops"""
    _run(ctx, entry)


@pytest.mark.parametrize("case", WALK, ids=lambda w: w.name)
def test_walk_case(ctx, case):
    """klt_min_distance_walk over a given list: key counts around the super-batches of 1024, more than 64 survivors in one, the list
    filling up at a super-batch's edges, no minimum distance, the cell grid in LDS and in global memory, cell sizes up to 257 with
    coordinates up to 65534, kept lists longer than 1024 slots"""
    bad = run_walk_trial(ctx, case)
    assert bad is None, bad


@pytest.mark.parametrize("seed", DRAW_SEEDS)
def test_pick_draw(ctx, seed):
    """a drawn lattice, radius, score form, mode and list length from the classes of the tables"""
    _run(ctx, draw_entry(seed))
