"""The selection-grid rule on the CPU: tests/select_grid_expected.py against the pinned oracle's own selection where the two must agree,
the properties the rule promises, what tc.selectionGrid accepts and refuses, and what the seeded draws cover.  No GPU."""
import numpy as np
import pytest

from oracle import klt_oracle as ko
from helpers import make_tc, params_from_tc
from select_grid_expected import (N_DRAWS, accepted_sequence, cells_of, grid_case, grid_dims, grid_facts, live_counts,
                                  select_grid_expected)
from select_mask_expected import (KLT_NOT_FOUND, REPLACING_SOME, SELECTING_ALL, drop_every_third, frame, same_records, select_expected)

W, H = 320, 240


@pytest.fixture(scope="module")
def case():
    p = params_from_tc(make_tc())
    img = frame(W, H).astype(np.float32)
    plain = ko.select_good_features(p, img, 100)
    start = drop_every_third(plain)
    return dict(p=p, img=img, plain=plain, start=start, A=accepted_sequence(p, img),
                A_rep=accepted_sequence(p, img, REPLACING_SOME, start))


def is_subsequence(part, whole):
    keys = {(float(a["x"]), float(a["y"]), int(a["val"])): i for i, a in enumerate(whole)}
    at = [keys.get((float(a["x"]), float(a["y"]), int(a["val"])), -1) for a in part]
    return all(i >= 0 for i in at) and all(a < b for a, b in zip(at, at[1:]))


def test_A_starts_with_the_plain_selection(case):
    assert len(case["A"]) > 100
    assert same_records(case["A"][:100], select_expected(case["p"], case["img"], 100))
    rep = select_expected(case["p"], case["img"], 100, REPLACING_SOME, case["start"])
    lost = case["start"]["val"] < 0
    assert same_records(case["A_rep"][:lost.sum()], rep[lost])


@pytest.mark.parametrize("q", [100, 101, 65535])
def test_one_cell_with_room_for_every_slot_is_the_plain_selection(case, q):
    got = select_grid_expected(case["p"], case["img"], 100, (W, H, q))
    assert got.tobytes() == case["plain"].tobytes()
    got = select_grid_expected(case["p"], case["img"], 100, (W + 77, H + 5, q), REPLACING_SOME, case["start"])
    want = ko.select_good_features(case["p"], case["img"], 100, REPLACING_SOME, case["start"].copy())
    assert got.tobytes() == want.tobytes()


def test_one_cell_of_k_keeps_the_first_k(case):
    k = 37
    got = select_grid_expected(case["p"], case["img"], 100, (W, H, k))
    assert same_records(got[:k], case["plain"][:k])
    assert (got["val"][k:] == KLT_NOT_FOUND).all() and (got["x"][k:] == -1).all() and (got["y"][k:] == -1).all()


@pytest.mark.parametrize("grid", [(64, 48, 3), (50, 70, 2), (33, 17, 1), (320, 7, 4)])
def test_no_cell_exceeds_the_quota_and_results_follow_A(case, grid):
    for n in (50, 100, 400):
        got = select_grid_expected(case["p"], case["img"], n, grid)
        found = got[got["val"] >= 0]
        assert live_counts(got, W, H, grid).max() <= grid[2]
        assert is_subsequence(found, case["A"])
        assert (got["val"][len(found):] == KLT_NOT_FOUND).all(), "the found records come first"
        # greedy: a member of A in front of the last one taken is missing only where its cell was full when the walk reached it
        if len(found):
            upto = [i for i, a in enumerate(case["A"]) if a["x"] == found[-1]["x"] and a["y"] == found[-1]["y"]][0]
            counts = np.zeros(np.prod(grid_dims(W, H, grid)), int)
            for a in case["A"][:upto + 1]:
                c = int(cells_of(int(a["x"]), int(a["y"]), W, grid))
                taken = bool(((found["x"] == a["x"]) & (found["y"] == a["y"])).any())
                assert taken == (counts[c] < grid[2])
                counts[c] += taken


def test_replacement_keeps_live_features_and_skips_full_cells(case):
    grid = (64, 48, 3)
    start = case["start"]
    live = start["val"] >= 0
    got = select_grid_expected(case["p"], case["img"], 100, grid, REPLACING_SOME, start)
    assert got[live].tobytes() == start[live].tobytes()
    before, after = live_counts(start, W, H, grid), live_counts(got, W, H, grid)
    at_capacity = before >= grid[2]
    assert at_capacity.any() and (before > grid[2]).any(), "no cell with more live features than the quota: the case shows nothing"
    assert (after[at_capacity] == before[at_capacity]).all(), "a cell with live >= q got a feature"
    assert (after[~at_capacity] <= grid[2]).all()
    new = got[~live & (got["val"] >= 0)]
    assert len(new) and is_subsequence(new, case["A_rep"])
    assert (got["val"][~live] < 0).any(), "lost slots stay lost where the kept members ran out"


def test_live_counts_ignore_what_lies_outside_the_frame():
    fl = ko.make_featurelist(6)
    fl["x"][:] = [5.9, -0.5, 320.0, np.nan, 63.99, 64.0]
    fl["y"][:] = [5.2, 3.0, 3.0, 3.0, 47.99, 48.0]
    fl["val"][:] = [1, 1, 1, 1, 0, 7]
    live = live_counts(fl, W, H, (64, 48, 3))
    assert live.sum() == 3 and live[0] == 2 and live[5 + 1] == 1


def test_select_grid_from_tc():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    from pyfeaturetrack_amd.params import select_grid_from_tc
    tc = KLT_TrackingContext()
    assert tc.selectionGrid is None and select_grid_from_tc(tc) is None
    assert select_grid_from_tc(object()) is None                           # read with a default, like tc.selectionMask
    for given in ((64, 48, 3), [1, 1, 1], np.array([50, 70, 65535]), (np.int32(8), np.int64(9), 2)):
        tc.selectionGrid = given
        got = select_grid_from_tc(tc)
        assert got == tuple(int(v) for v in given) and all(type(v) is int for v in got)
    for bad in (5, "abc", (64, 48), (64, 48, 3, 1), (64.0, 48, 3), (64, 48, None), (True, 48, 3), {"w": 1}, b"abc"):
        tc.selectionGrid = bad
        with pytest.raises(TypeError):
            select_grid_from_tc(tc)
    for bad in ((0, 48, 3), (64, 0, 3), (-1, 48, 3), (64, 48, 0), (64, 48, 65536), (64, 48, -2), (2 ** 31, 4, 1)):
        tc.selectionGrid = bad
        with pytest.raises(ValueError):
            select_grid_from_tc(tc)


def test_the_draws_cover_what_they_are_for():
    facts = [dict(grid_facts(grid_case(k)), **grid_case(k)["t"]) for k in range(N_DRAWS)]
    for f in facts:
        c = grid_case(f["k"])
        assert live_counts(c["want"], f["w"], f["h"], c["grid"]).max() <= max(
            f["q"], live_counts(c["start"], f["w"], f["h"], c["grid"]).max() if c["start"] is not None else 0)
    assert any(f["full"] for f in facts) and any(not f["full"] for f in facts)
    assert any(f["capped"] for f in facts) and any(f["uncapped"] for f in facts) and any(not f["capped"] for f in facts)
    assert any(f["partial"] for f in facts)
    for mode in (SELECTING_ALL, REPLACING_SOME):
        assert any(f["mode"] == mode and f["capped"] and f["placed"] > 0 for f in facts), mode
    for mindist in (0, 1):
        assert any(f["mindist"] == mindist and f["capped"] for f in facts), mindist
    assert any(f["skip"] > 0 and f["capped"] for f in facts)
    assert any(f["masked"] and f["capped"] for f in facts) and any(f["q"] > 64 and f["capped"] for f in facts)
