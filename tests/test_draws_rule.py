"""The seed tables of tests/draws_expected.py cover what they claim (no GPU): the expected records of every entry are computed with the
CPU oracle alone and the conditions below asserted on them.  These are conditions, not measurements: a seed that fails one is replaced in
the table."""
import numpy as np
import pytest

from draws_expected import (FB_MAX_ERRORS, KLT_FB_INCONSISTENT, KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS, KLT_OOB, KLT_SMALL_DET, KLT_TRACKED,
                            MASK_LARGE_SEEDS, MASK_SEEDS, MAX_PIXELS, PREFILTER_CANDIDATES, QUAD_FEATURES, REPLACING_SOME, TRACK_SEEDS, WINDOWS, draw_mask, draw_track, mask_case,
                            mask_facts, track_case, track_facts)


def test_table_sizes_and_draw_ranges():
    assert len(TRACK_SEEDS) == len(set(TRACK_SEEDS)) == 24 and len(MASK_SEEDS) == len(set(MASK_SEEDS)) == 16
    for seed in range(300):                        # the draws stay inside the parameter space, whatever the seed
        t = draw_track(seed)
        coarse = t["ss"] ** (t["levels"] - 1)
        assert 48 <= t["w"] <= 360 and 48 <= t["h"] <= 360 and t["w"] * t["h"] <= MAX_PIXELS
        assert t["w"] // coarse >= t["window"] + 12 and t["h"] // coarse >= t["window"] + 12
        assert t["window"] in WINDOWS and 1 <= t["levels"] <= 4 and t["ss"] in (2, 4, 8) and t["fb_max_error"] in FB_MAX_ERRORS
        assert t["border"] is None or t["window"] // 2 + 1 <= t["border"] <= 40
        assert t["n"] % 4 != 0 and (1 <= t["n"] <= 600 or (t["window"] == 7 and t["scattered"] and QUAD_FEATURES < t["n"] <= 2300))
        length = np.hypot(*t["shift"])
        assert (10.0 <= length <= 60.0) if t["far"] else (abs(t["shift"][0]) <= 3 and abs(t["shift"][1]) <= 3)
        m = draw_mask(seed)
        assert 48 <= m["w"] <= 360 and 48 <= m["h"] <= 360 and m["w"] * m["h"] <= MAX_PIXELS
        assert 3 <= m["window"] <= 15 and 0 <= m["skip"] <= 3 and 0 <= m["mindist"] <= 25 and 1 <= m["n"] <= 600


def test_tracking_table():
    facts = {seed: track_facts(track_case(seed)) for seed in TRACK_SEEDS}
    draws = {seed: track_case(seed)["t"] for seed in TRACK_SEEDS}
    assert {t["window"] for t in draws.values()} == set(WINDOWS)
    assert {t["levels"] for t in draws.values()} == {1, 2, 3, 4}
    assert {t["ss"] for t in draws.values()} == {2, 4, 8}
    seen = set().union(*(f["statuses"] for f in facts.values()))
    assert {KLT_TRACKED, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_OOB, KLT_LARGE_RESIDUE, KLT_FB_INCONSISTENT} <= seen, seen
    assert any(f["nibble15"] for f in facts.values()), "no aux nibble saturates"
    assert any(f["unvisited"] for f in facts.values()), "no feature stops with unvisited levels"
    # both kinds of list, the dense 7x7 lists (a single launch on the four-feature kernel) with and without a far shift
    assert any(t["scattered"] for t in draws.values()) and any(not t["scattered"] for t in draws.values())
    assert any(t["n"] > QUAD_FEATURES and t["far"] for t in draws.values()) and any(t["n"] > QUAD_FEATURES and not t["far"] for t in draws.values())
    # the windows that never met a prior before: each in a far draw (the any-window kernel with 1, 4 and 8 and more samples per lane)
    assert {3, 5, 11, 13, 17, 21} <= {t["window"] for t in draws.values() if t["far"]}
    assert {1, 4} <= {t["levels"] for t in draws.values() if t["far"]} and 8 in {t["ss"] for t in draws.values() if t["far"]}
    for seed, f in facts.items():
        assert 4 * f["tracked"] >= f["live"] > 0, (seed, f)
        if draws[seed]["far"]:
            assert f["prior_differs"] >= 10, (seed, f)
    assert 2 * sum(f["keeps_and_rejects"] for f in facts.values()) >= len(facts)


@pytest.mark.parametrize("seed", TRACK_SEEDS)
def test_tracking_draw_inputs(seed):
    """what the issue rules out of the input list stays out: finite positions on the image"""
    c = track_case(seed)
    t, fin, g = c["t"], c["fin"], c["guess"]
    live = fin["val"] >= 0
    assert np.isfinite(fin["x"]).all() and np.isfinite(fin["y"]).all() and len(fin) == t["n"]
    assert (fin["x"][live] >= 0).all() and (fin["x"][live] <= t["w"] - 1).all() and (fin["y"][live] >= 0).all() and (fin["y"][live] <= t["h"] - 1).all()
    assert (~live).any() or t["n"] < 20
    counts = live & (g["val"] >= 0) & np.isfinite(g["x"]) & np.isfinite(g["y"])
    if t["n"] >= 100:                              # the guess list mixes guesses that count, that do not, and that lie off the image
        off = counts & ((g["x"] < 0) | (g["y"] < 0) | (g["x"] > t["w"] - 1) | (g["y"] > t["h"] - 1))
        assert counts.any() and (live & ~counts).any() and off.any()
        assert (c["guessed"]["val"][off] == KLT_OOB).all()


def test_mask_table():
    facts = {seed: mask_facts(mask_case(seed)) for seed in MASK_SEEDS}
    draws = {seed: mask_case(seed)["t"] for seed in MASK_SEEDS}
    for seed, f in facts.items():
        assert f["differs"], "seed %d: the mask changes nothing" % seed
        assert not f["on_zero"], "seed %d: a feature was placed on a masked pixel" % seed
    assert sum(f["tail_zero"] for f in facts.values()) >= 4
    assert sum(f["live_overlap"] and draws[s]["mode"] == REPLACING_SOME for s, f in facts.items()) >= 4
    assert 3 * sum(f["n16"] != 0 for f in facts.values()) >= len(facts) and len({f["n16"] for f in facts.values()}) >= 6
    assert {t["skip"] for t in draws.values()} == {0, 1, 2, 3}
    assert {t["kind"] for t in draws.values()} >= {"rectangles", "bernoulli", "sparse", "lines", "window"}
    assert any(t["any_value"] for t in draws.values()) and any(not t["smooth"] for t in draws.values())
    assert any(0 < f["placed"] < draws[s]["n"] for s, f in facts.items()), "the candidates never run out"


def test_large_mask_table():
    """the frames above the prefilter's threshold: more than 262144 candidates each, both modes, nSkippedPixels 0 and 1, and the same
    conditions as the small table's entries"""
    from oracle import klt_oracle as ko
    cases = [mask_case(seed, True) for seed in MASK_LARGE_SEEDS]
    for c in cases:
        t, f = c["t"], mask_facts(c)
        bx, by, _, _ = ko.scan_borders(c["p"])
        step = t["skip"] + 1
        cells = ((t["w"] - 2 * bx + step - 1) // step) * ((t["h"] - 2 * by + step - 1) // step)
        assert cells > PREFILTER_CANDIDATES and max(65536, 64 * t["n"]) < cells // 2, (t, cells)
        assert f["differs"] and not f["on_zero"], t
    assert {c["t"]["mode"] for c in cases} == {1, REPLACING_SOME} and {c["t"]["skip"] for c in cases} == {0, 1}
    assert any(c["t"]["mode"] == REPLACING_SOME and c["t"]["mindist"] > 0 and mask_facts(c)["live_overlap"] for c in cases)
