"""The crowding check's rule (include/klt_gpu.h) without a GPU: tests/crowd_expected.py, the restatement the device
is compared with, against the reference's own minimum-distance walk (oracle/min_distance_walk.py) and against the parallel-rounds form
the kernels use; the rule's corner cases; crowd_params_from_tc."""
import numpy as np
import pytest

from crowd_expected import (CROWD_DTYPE, INT32_MAX, KLT_CROWDED, border_pairs, candidate_mask, chain, crowd_check_expected, crowd_records,
                            live_pairs_within, non_candidate_kinds, parallel_rounds, pixels, priority_order, random_list, records, ages_in,
                            serial_walk, zoom_out_geometry)
from helpers import make_tc

NCOLS, NROWS = 320, 240


def walk_inputs(out, prev, ncols=NCOLS, nrows=NROWS):
    cand = candidate_mask(out, ncols, nrows)
    px, py = pixels(out, cand)
    return px, py, priority_order(cand, ages_in(prev, len(out)))


def lists():
    made = [("random %d, d %d" % (n, d), random_list(n, NCOLS, NROWS, seed=n + d), d)
            for n, d in ((300, 1), (300, 2), (300, 10), (300, 33), (2000, 2), (2000, 10))]
    made.append(("chain", chain(60, 9), 10))
    made.append(("chain, reversed", chain(60, 9, reverse=True), 10))
    made.append(("diagonal chain", chain(25, 9, dx=1, dy=1), 10))
    return made


@pytest.mark.parametrize("name,pair,d", lists(), ids=[m[0] for m in lists()])
def test_the_restatement_is_the_reference_walk(name, pair, d):
    """offered the candidates' pixels as a point list in priority order, the reference's walk accepts exactly the kept ones, in order"""
    from oracle.min_distance_walk import enforce_minimum_distance
    out, prev = pair
    px, py, order = walk_inputs(out, prev)
    verdict = serial_walk(px, py, order, d - 1)
    kept = [int(i) for i in order if verdict[int(i)] < 0]
    points = [(1, int(px[i]), int(py[i])) for i in order]
    feats = enforce_minimum_distance(points, [[-1, -1, -1] for _ in order], NCOLS, NROWS, d, 1, True)
    accepted = [(f[0], f[1]) for f in feats if f[2] >= 0]
    assert accepted == [(int(px[i]), int(py[i])) for i in kept]
    assert all(f[2] < 0 for f in feats[len(kept):])
    # the winner of a crowded one is a kept one that covers it, and no earlier kept one does
    rank = {int(i): k for k, i in enumerate(order)}
    for i, w in verdict.items():
        if w >= 0:
            assert verdict[w] < 0 and rank[w] < rank[i] and abs(px[i] - px[w]) <= d - 1 and abs(py[i] - py[w]) <= d - 1
            assert not any(rank[j] < rank[w] and abs(px[i] - px[j]) <= d - 1 and abs(py[i] - py[j]) <= d - 1 for j in kept)
    if d > 1 and name.startswith("random"):
        assert any(w >= 0 for w in verdict.values())


@pytest.mark.parametrize("name,pair,d", lists(), ids=[m[0] for m in lists()])
def test_the_parallel_rounds_give_the_serial_walk(name, pair, d):
    out, prev = pair
    px, py, order = walk_inputs(out, prev)
    verdict = serial_walk(px, py, order, d - 1)
    state, rounds = parallel_rounds(px, py, order, d - 1)
    assert {i: w < 0 for i, w in verdict.items()} == state
    print("%s: %d candidates, %d rounds" % (name, len(order), rounds))
    if "chain" in name:
        assert rounds == len(order)                          # data-dependent: a loop over rounds must end on a condition
    else:
        assert rounds <= 12


def test_equal_ages_are_decided_by_index_and_identical_positions_keep_the_lowest():
    out = records([50.2, 50.9, 50.5, 120.0], [60.1, 60.7, 60.0, 60.0])
    want, crowd = crowd_check_expected(out, None, NCOLS, NROWS, 1)          # r = 0: the same pixel only
    assert crowd["val"].tolist() == [1, 2, 2, 1] and crowd["winner"].tolist() == [-1, 0, 0, -1]
    assert want["val"].tolist() == [0, KLT_CROWDED, KLT_CROWDED, 0] and want["x"].tolist() == [np.float32(50.2), -1, -1, 120]
    want, crowd = crowd_check_expected(out, crowd_records([3, 3, 3, 3]), NCOLS, NROWS, 1)
    assert crowd["val"].tolist() == [1, 2, 2, 1] and crowd["age"].tolist() == [4, 0, 0, 4]
    want, crowd = crowd_check_expected(out, crowd_records([0, 1, 5, 0]), NCOLS, NROWS, 1)     # the oldest wins, whatever its index
    assert crowd["val"].tolist() == [2, 2, 1, 1] and crowd["winner"].tolist() == [2, 2, -1, -1]


def test_negative_ages_count_as_zero_and_age_saturates():
    out = records([10, 12, 100, 200], [10, 10, 10, 10])
    _, crowd = crowd_check_expected(out, crowd_records([-5, 0, INT32_MAX, INT32_MAX - 1]), NCOLS, NROWS, 10)
    assert crowd["val"].tolist() == [1, 2, 1, 1]             # -5 counts as 0: index decides against record 1
    assert crowd["age"].tolist() == [1, 0, INT32_MAX, INT32_MAX]
    assert crowd.dtype == CROWD_DTYPE and (crowd["pad"] == 0).all()


def test_non_candidates_keep_their_bytes_and_aux_survives():
    out, prev = random_list(600, NCOLS, NROWS, seed=3)
    non, edge = non_candidate_kinds(out, NCOLS, NROWS, start=1, step=16)
    assert len(non) >= 20 and len(edge) == 4
    want, crowd = crowd_check_expected(out, prev, NCOLS, NROWS, 10)
    assert want[non].tobytes() == out[non].tobytes() and (crowd["val"][non] == 0).all() and (crowd["winner"][non] == -1).all()
    assert (crowd["val"][edge] > 0).all()
    flagged = crowd["val"] == 2
    assert flagged.sum() > 100 and (want["aux"] == out["aux"]).all() and (want["val"][flagged] == KLT_CROWDED).all()
    assert want[~flagged].tobytes() == out[~flagged].tobytes()


@pytest.mark.parametrize("d", [1, 2, 10, 33])
def test_the_check_on_its_own_output_flags_nothing_further(d):
    out, prev = random_list(800, NCOLS, NROWS, seed=d)
    want, crowd = crowd_check_expected(out, prev, NCOLS, NROWS, d)
    assert live_pairs_within(want, d - 1, NCOLS, NROWS) == 0
    again, crowd2 = crowd_check_expected(want, crowd, NCOLS, NROWS, d)
    assert again.tobytes() == want.tobytes() and not (crowd2["val"] == 2).any()
    kept = crowd["val"] == 1
    assert (crowd2["age"][kept] == crowd["age"][kept] + 1).all() and (crowd2["val"][~kept] == 0).all()


def test_border_pairs_are_decided_by_the_distance_alone():
    out, _ = border_pairs(NCOLS, NROWS, 9, 16)
    _, crowd = crowd_check_expected(out, None, NCOLS, NROWS, 10)
    assert crowd["val"].tolist() == [1, 2] * 3 + [1, 1] * 3 + [1, 1]


def test_the_zoom_out_geometry_crowds_without_the_check():
    """the inputs exercise the feature: a lattice 10 px apart, scaled as the clip's frames are, has live pairs within r after a few frames"""
    pairs = zoom_out_geometry(12, NCOLS, NROWS, 10, 10)
    print("live pairs within 9 px per frame:", pairs)
    assert pairs[0] == 0 and pairs[-1] > 100 and all(b >= a for a, b in zip(pairs, pairs[1:]))


def test_crowd_params_from_tc():
    from pyfeaturetrack_amd.params import age_records, crowd_params_from_tc
    tc = make_tc()
    assert crowd_params_from_tc(tc).mode == 0 and tc.crowdingCheck is False and tc.crowding_min_distance is None
    del tc.crowdingCheck, tc.crowding_min_distance           # a tracking context made elsewhere has neither
    assert crowd_params_from_tc(tc).mode == 0
    tc.crowdingCheck = True
    cp = crowd_params_from_tc(tc, 320, 240)
    assert (cp.mode, cp.ncols, cp.nrows, cp.min_distance) == (1, 320, 240, tc.mindist)
    tc.crowding_min_distance = 4
    assert crowd_params_from_tc(tc, 320, 240).min_distance == 4
    tc.lightingCompensation = "gain_bias"                    # it reads no frame: goes with lighting compensation
    assert crowd_params_from_tc(tc, 320, 240).mode == 1
    for bad in (0, -3, 2.5, True):
        tc.crowding_min_distance = bad
        with pytest.raises(ValueError):
            crowd_params_from_tc(tc)
    tc.crowding_min_distance = None
    for bad in (1, 0, "yes", None):
        tc.crowdingCheck = bad
        with pytest.raises(ValueError):
            crowd_params_from_tc(tc)
    tc.crowdingCheck = True
    tc.affineConsistencyCheck = 0
    with pytest.raises(ValueError):
        crowd_params_from_tc(tc)
    tc.affineConsistencyCheck = -1
    with pytest.raises(ValueError):
        crowd_params_from_tc(tc, 70000, 240)
    assert age_records(None, 5) is None
    rec = age_records([3, 0, 7], 3)
    assert rec.view(CROWD_DTYPE).reshape(3)["age"].tolist() == [3, 0, 7]
    for bad in ([1, 2], [1.0, 2.0, 3.0], [[1, 2, 3]]):
        with pytest.raises(ValueError):
            age_records(bad, 3)
