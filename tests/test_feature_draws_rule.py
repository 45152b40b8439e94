"""The seed tables of tests/feature_draws_expected.py reach what they are there for (no GPU): the expected records of every entry are
computed with the numpy restatements alone and the conditions below asserted on them.  These are conditions, not measurements: a seed that
fails one is replaced in the table, never skipped at run time.  tests/COVERAGE.md says which entry reaches which kernel instantiation
and loop edge, and lists what no input reaches."""
import numpy as np
import pytest

from feature_draws_expected import (F32_BLOCKS, GATHER_TILE, LIGHT_SEEDS, LIGHT_WINDOWS, MODEL_EDGE_NAMES, MODEL_HYPOTHESES,
                                    MODEL_LENGTHS, MODEL_M_EDGES, MODEL_SEEDS, N_UNMEASURED_KINDS, QUALITY_KINDS, QUALITY_SEEDS, QUAD_FEATURES,
                                    WINDOW_CLASSES, differ, draw_light, draw_model, draw_quality, light_case, light_facts, light_path,
                                    model_case, model_differ, model_edge_case, model_facts, probed_light_level, probed_quality_record,
                                    quality_case, quality_differ, quality_facts)
from draws_expected import MAX_PIXELS
from light_expected import KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS, KLT_OOB, KLT_SMALL_DET, KLT_TRACKED


def test_draw_ranges():
    """the draws stay inside the parameter space, whatever the seed"""
    for seed in range(300):
        for t in (draw_light(seed), draw_quality(seed)):
            coarse = t["ss"] ** (t["levels"] - 1)
            assert t["window"] == LIGHT_WINDOWS[seed % 14] and 1 <= t["levels"] <= 4 and t["ss"] in (2, 4, 8)
            assert t["w"] * t["h"] <= MAX_PIXELS and t["w"] // coarse >= t["window"] + 12 and t["h"] // coarse >= t["window"] + 12
            assert 2 <= t["npairs"] <= 4 and t["n"] <= 2300 and t["dtype"] in ("u8", "f32")
        t = draw_light(seed)
        assert t["block_kind"] in F32_BLOCKS and (t["dtype"] == "f32" or t["block_kind"] in F32_BLOCKS[:4])
        assert 255.0 * t["gain"] + t["offset"] <= 255.0 and t["max_iter"] in (3, 10, 25)
        if t["form"] == "below":
            assert t["window"] == 7 and QUAD_FEATURES - 4 <= t["n"] * t["npairs"] < QUAD_FEATURES
        if t["form"] == "above":
            assert t["window"] == 7 and t["n"] < QUAD_FEATURES <= t["n"] * t["npairs"] <= QUAD_FEATURES + 1
        q = draw_quality(seed)
        assert q["kind"] in QUALITY_KINDS and q["n"] >= q["kinds_start"] + N_UNMEASURED_KINDS
        m = draw_model(seed)
        assert 1 <= m["n"] <= 20000 and 64 <= m["ncols"] <= 65535 and 64 <= m["nrows"] <= 65535 and 2 <= m["npairs"] <= 4
        assert m["params"]["hypotheses"] in MODEL_HYPOTHESES and 0 <= m["params"]["seed"] <= 0xffffffff


# ---------------------------------------------------------------------------------------------------------------- gain / bias tracking
@pytest.fixture(scope="module")
def light_table():
    return {seed: (light_case(seed)["t"], light_facts(light_case(seed))) for seed in LIGHT_SEEDS}


def test_light_table(light_table):
    draws = [t for t, _ in light_table.values()]
    facts = [f for _, f in light_table.values()]
    assert len(LIGHT_SEEDS) == len(set(LIGHT_SEEDS))
    assert {f["cls"] for f in facts} == WINDOW_CLASSES                              # every instantiation of track_light_kernel
    assert {t["window"] for t in draws} == set(LIGHT_WINDOWS)
    assert {t["levels"] for t in draws} == {1, 2, 3, 4} and {t["ss"] for t in draws} == {2, 4, 8}
    assert {t["dtype"] for t in draws} == {"u8", "f32"}
    assert {t["block_kind"] for t in draws} == set(F32_BLOCKS)
    # the four-feature kernel on single lists with n % 4 of 0, 1, 2, 3, and the wave kernel one feature below its threshold
    assert {t["n"] % 4 for t in draws if light_path(t, 4, 1) == 2} == {0, 1, 2, 3}
    assert any(t["n"] == QUAD_FEATURES - 1 and t["window"] == 7 for t in draws)
    # batches on either side of the threshold.  2047 = 23 * 89: no batch of 2 - 4 pairs has that many features, so the product of exactly
    # 2047 is a batch of one pair (every trial launches one), and the largest product of 2 - 4 pairs below 2048 is 2046 or 2044
    assert any(t["window"] == 7 and t["n"] < QUAD_FEATURES <= t["n"] * t["npairs"] for t in draws)
    assert any(t["window"] == 7 and t["n"] * 1 == QUAD_FEATURES - 1 for t in draws)
    assert any(t["window"] == 7 and t["n"] * t["npairs"] in (QUAD_FEATURES - 2, QUAD_FEATURES - 4) for t in draws)
    for seed, (t, f) in light_table.items():
        assert f["tracked"] >= 10 and f["lost"] >= 5, (seed, f)
    seen = set().union(*(f["statuses"] for f in facts))
    assert {KLT_TRACKED, KLT_OOB, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_LARGE_RESIDUE} <= seen, seen
    assert any(f["nibble15"] for f in facts), "no aux nibble saturates"
    assert any(f["unvisited"] for f in facts), "no feature stops with unvisited levels"
    assert any(f["not_positive"] for f in facts), "no window is degenerate by a sum that is not positive"
    assert any(f["overflowed"] for f in facts), "no window is degenerate by a sum or square that overflowed"
    assert any(f["step_not_finite"] for f in facts), "no Newton step is not finite behind sums that passed"
    # each of the three on a draw of its own kind
    by_kind = {t["block_kind"]: f for t, f in light_table.values()}
    assert by_kind["negative"]["not_positive"] and by_kind["overflow"]["overflowed"] and by_kind["bright"]["step_not_finite"]


def test_light_extremes_form_no_position(light_table):
    """the float32 extreme blocks are data the kernels' guards are written for: no expected record holds a position that is not finite"""
    for seed in LIGHT_SEEDS:
        for want in light_case(seed)["want"]:
            assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all(), seed


def test_light_probe_counts_what_it_says():
    """the probed copy of light_level on planes made for each branch: a flat positive pair (nothing counted), image 2 negative, image 2 so
    bright that its squares overflow, both so bright that the determinant's products do"""
    import light_expected as le
    from helpers import make_tc, params_from_tc
    p = params_from_tc(make_tc(levels=1, ss=2, window=5))
    rs = np.random.RandomState(3)
    img = rs.uniform(50, 200, (40, 40)).astype(np.float32)
    gy, gx = (g.astype(np.float32) for g in np.gradient(img))
    x = np.full(4, 20.25, np.float32)
    for scale1, scale2, want in ((1.0, 1.0, {}), (1.0, -1.0, {"not_positive": 4}), (1.0, 2.0 ** 65, {"overflowed": 4}),
                                 (2.0 ** 40, 2.0 ** 40, {"step_not_finite": 4})):
        counts = {}
        with probed_light_level(counts):
            lv1, lv2 = [pl * np.float32(scale1) for pl in (img, gx, gy)], [pl * np.float32(scale2) for pl in (img, gx, gy)]
            val, _, _, it = le.light_level(p, lv1, lv2, x, x, x + np.float32(0.5), x)
        assert {k: v for k, v in counts.items() if v} == want, (scale1, scale2, counts)
        assert (val == (KLT_SMALL_DET if want else KLT_TRACKED)).all(), (scale1, scale2, val)


# ------------------------------------------------------------------------------------------------------------------------ track quality
@pytest.fixture(scope="module")
def quality_table():
    return {seed: (quality_case(seed)["t"], quality_facts(quality_case(seed))) for seed in QUALITY_SEEDS}


def test_quality_table(quality_table):
    draws = [t for t, _ in quality_table.values()]
    facts = [f for _, f in quality_table.values()]
    assert len(QUALITY_SEEDS) == len(set(QUALITY_SEEDS))
    assert {f["cls"] for f in facts} == WINDOW_CLASSES and {t["window"] for t in draws} == set(LIGHT_WINDOWS)
    assert {t["dtype"] for t in draws} == {"u8", "f32"} and {t["kind"] for t in draws} == set(QUALITY_KINDS)
    assert {t["w"] % 4 for t in draws} == {0, 1, 2, 3} and {t["npairs"] for t in draws} == {2, 3, 4}
    for seed, (t, f) in quality_table.items():
        assert f["measured"] >= 40 and f["unmeasured"] >= 20, (seed, f)
    assert set().union(*(f["kinds"] for f in facts)) == set(range(N_UNMEASURED_KINDS))     # every kind of unmeasured_kinds, somewhere
    total = {k: sum(f.get(k, 0) for f in facts) for k in ("a_le_0", "b_le_0", "e_le_0", "clamp_high", "clamp_low", "ncc_is_1")}
    print("quality branches over the table:", total)
    assert total["a_le_0"] and total["b_le_0"] and total["e_le_0"], total
    assert total["ncc_is_1"], total                     # identical windows: exactly on the upper clamp's bound, not behind it
    assert total["clamp_high"] and total["clamp_low"], total                    # the "gained" and "negated" pairs at 3x3 windows
    by_kind = {t["kind"]: f for t, f in quality_table.values() if t["window"] == 3}
    assert by_kind["gained"]["clamp_high"] and by_kind["negated"]["clamp_low"]


def test_quality_probe_counts_what_it_says():
    """the probed copy of quality_record on prepared windows: equal windows sit exactly on 1, windows equal up to a rounded gain land on
    either side of +-1 (by Cauchy-Schwarz |c| <= sqrt(a * b) in exact arithmetic: only the rounding of the quotient passes the bound),
    constant windows take the a <= 0 / b <= 0 branch, windows without gradients the e <= 0 branch"""
    import quality_expected as qe

    class Sampler:                                  # stands for the oracle: hands out prepared windows instead of sampling a frame
        def __init__(self):
            self.queue = []

        def extract_patch(self, img, x, y, w, h):
            return self.queue.pop(0)

        @staticmethod
        def abs_sum_f32(d):
            return np.abs(d).sum(dtype=np.float32)

    rs = np.random.RandomState(11)
    ko = Sampler()
    fin, fout = np.array((40.0, 40.0, 1, 0), qe.FEAT_DTYPE), np.array((40.0, 40.0, 0, 0), qe.FEAT_DTYPE)
    img = np.zeros((80, 80), np.float32)
    seen = {}
    for kind in ("equal", "gained", "negated", "constant"):
        counts = seen.setdefault(kind, {})
        with probed_quality_record(counts):
            for trial in range(400):
                w = (3, 7, 13)[trial % 3]
                T = rs.uniform(0, 255, (w, w)).astype(np.float32)
                gain = {"equal": 1.0, "gained": rs.uniform(0.1, 3.0), "negated": -rs.uniform(0.1, 3.0), "constant": 1.0}[kind]
                if kind == "constant":
                    T = np.full((w, w), 117, np.float32)
                S = (T.astype(np.float64) * gain).astype(np.float32)
                g = np.zeros((w, w), np.float32)
                ko.queue = [T, S, g, g]
                rec = qe.quality_record(ko, img, img, img, img, fin, fout, w)
                assert -1.0 <= rec[1] <= 1.0 and rec[2] == 0 and rec[3] == 1
    print("prepared windows:", seen)
    assert seen["equal"]["ncc_is_1"] == 400 and seen["equal"]["clamp_high"] == 0 and seen["equal"]["e_le_0"] == 400
    assert seen["gained"]["clamp_high"] > 0 and seen["gained"]["clamp_low"] == 0
    assert seen["negated"]["clamp_low"] > 0 and seen["negated"]["clamp_high"] == 0
    assert seen["constant"]["a_le_0"] == 400 and seen["constant"]["b_le_0"] == 400 and "clamp_high" not in seen["constant"]


# ------------------------------------------------------------------------------------------------------------------- motion-model check
@pytest.fixture(scope="module")
def model_table():
    table = {("draw", seed): model_case(seed) for seed in MODEL_SEEDS}
    table.update({("edge", name): model_edge_case(name) for name in MODEL_EDGE_NAMES})
    return {k: (c["t"], model_facts(c)) for k, c in table.items()}


def test_model_tables(model_table):
    edges = {k[1]: v for k, v in model_table.items() if k[0] == "edge"}
    every = [f for _, facts in model_table.values() for f in facts]
    assert len(MODEL_SEEDS) == len(set(MODEL_SEEDS))
    assert {n for n in MODEL_LENGTHS} <= {t["n"] for t, _ in edges.values()}
    assert MODEL_LENGTHS == [8191, 8192, 8193, 12289, 16384, 16385, 20000] and MODEL_M_EDGES == [255, 256, 257, 511, 512, 513, 2047, 2048, 2049]
    assert set(MODEL_M_EDGES) <= {facts[0]["m"] for _, facts in edges.values()}
    for m in MODEL_M_EDGES:
        assert edges["m%d" % m][1][0]["m"] == m and edges["m%d" % m][1][0]["valid"] == 1
    first, second, rounds = edges["first_tile_empty"][1][0], edges["second_tile_empty"][1][0], edges["rounds_4_to_7"][1][0]
    assert first["tile_candidates"][0] == 0 and first["tile_candidates"][1] >= 100 and first["valid"] == 1
    assert second["tile_candidates"][1] == 0 and second["tile_candidates"][0] >= 100 and second["valid"] == 1
    c = model_edge_case("rounds_4_to_7")
    from model_expected import candidate_mask
    cand = candidate_mask(c["pairs"][0], c["pairs"][1], c["t"]["ncols"], c["t"]["nrows"])
    assert not cand[:GATHER_TILE // 2].any() and cand[GATHER_TILE // 2:GATHER_TILE].sum() >= 4000 and cand[GATHER_TILE:GATHER_TILE * 3 // 2].sum() >= 4000
    # frame sizes that fill either half of the size word: bit 31 of the record's `pad` is set
    for name in ("size_65535x65535", "size_640x40000"):
        assert int(model_edge_case(name)["want_model"][0]["pad"]) < 0 and edges[name][1][0]["valid"] == 1
    assert [f["valid"] for f in edges["batch_of_every_outcome"][1]] == [0, 0, 1, 2]
    few, below, _, kept = edges["batch_of_every_outcome"][1]
    assert few["m"] < 8 and below["below"] and kept["tie"]
    assert {f["valid"] for f in every} == {0, 1, 2}
    assert any(f["tie"] and f["tie_winner"] > 0 for f in every), "no two hypotheses share the top score with the smaller one winning"
    assert any(f["tie"] and t["params"]["hypotheses"] > 512 for t, facts in model_table.values() for f in facts)
    assert any(f["below"] for f in every)
    seeds = {t["params"]["seed"] for t, _ in model_table.values()}
    assert {0x80000000, 0xffffffff} <= seeds and 0 in seeds and any(0x80000000 < s < 0xffffffff for s in seeds)
    assert {t["params"]["hypotheses"] for t, _ in model_table.values()} >= set(MODEL_HYPOTHESES)
    assert any(len(f["tile_candidates"]) == 3 for f in every) and any(t["n"] > GATHER_TILE and k[0] == "draw" for k, (t, _) in model_table.items())
    for key, (t, facts) in model_table.items():
        for f in facts:
            if f["valid"] == 1:
                assert f["flagged"] >= 1 and f["kept"] >= 1, (key, f)
            # valid == 2 keeps a hypothesis whose D is exactly 0: every residual is a sum of products with 0 and every candidate an
            # inlier, so such a model flags nothing (the rule's own arithmetic)
            if f["valid"] == 2:
                assert f["flagged"] == 0 and f["kept"] == f["m"], (key, f)


# ------------------------------------------------------------------------------------------------------------------------- sensitivity
def _flip(a, field, i):
    b = a.copy()
    bits = b[field].view(np.int32)
    bits[i] ^= 1
    return b


def _swap(a, i, j):
    b = a.copy()
    b[[i, j]] = b[[j, i]]
    return b


def test_the_comparisons_notice_one_bit_and_one_swap():
    """each of the three comparison functions reports one flipped low mantissa bit in one field of one record, and two records swapped"""
    c = light_case(LIGHT_SEEDS[0])
    want = c["want"][0]
    tracked = np.flatnonzero(want["val"] == KLT_TRACKED)
    assert differ(want.copy(), want, "same") is None
    for field in ("x", "y", "aux"):
        assert differ(_flip(want, field, tracked[3]), want, "flip") is not None, field
    assert differ(_swap(want, tracked[0], tracked[1]), want, "swap") is not None

    q = quality_case(QUALITY_SEEDS[0])["want"][0]
    measured = np.flatnonzero(q["val"] == 1)
    assert quality_differ(q.copy(), q, "same") is None
    for field in ("residue", "ncc", "min_eig", "val"):
        assert quality_differ(_flip(q, field, measured[2]), q, "flip") is not None, field
    assert quality_differ(_swap(q, measured[0], measured[1]), q, "swap") is not None
    zero = q.copy()
    zero["ncc"][np.flatnonzero(q["val"] == 0)[0]] = -0.0                          # -0 is not +0
    assert quality_differ(zero, q, "minus zero") is not None

    m = model_edge_case("n8193")
    out, model = m["want_out"][0], m["want_model"][0]
    kept = np.flatnonzero(out["val"] == KLT_TRACKED)
    assert model_differ(out.copy(), model.copy(), out, model, "same") is None
    assert model_differ(_flip(out, "x", kept[-1]), model, out, model, "flip") is not None           # (a record of the second tile)
    assert kept[-1] >= GATHER_TILE or kept[-2] >= GATHER_TILE - 1
    assert model_differ(_swap(out, kept[0], kept[-1]), model, out, model, "swap") is not None
    for field in ("nxx", "nty", "d"):
        rec = np.array(model)
        rec[field] = np.nextafter(rec[field], np.inf)
        assert model_differ(out, rec, out, model, "model") is not None, field
    rec = np.array(model)
    rec["n_inliers"] += 1
    assert model_differ(out, rec, out, model, "count") is not None


def test_a_gather_that_forgets_its_base_is_seen():
    """the mistake the lists above 8192 records are there for: candidate numbers that start again at 0 in every tile of the gather put the
    second tile's candidates over the first's.  Restated on the host for the table's n8193 entry, the expected records differ."""
    from model_expected import candidate_mask, motion_check_expected
    c = model_edge_case("n8193")
    t, fin, fout = c["t"], c["pairs"][0], c["pairs"][1]
    cand = np.flatnonzero(candidate_mask(fin, fout, t["ncols"], t["nrows"]))
    second = cand[cand >= GATHER_TILE]
    assert 1 <= second.size < GATHER_TILE
    bin_, bout = fin.copy(), fout.copy()
    first = cand[:second.size]                      # numbers 0 .. of the first tile, overwritten by the second tile's candidates
    bin_[first], bout[first] = fin[second], fout[second]
    got_out, got_model = motion_check_expected(bin_, bout, t["ncols"], t["nrows"], **t["params"])
    assert model_differ(got_out, got_model, c["want_out"][0], c["want_model"][0], "no base") is not None
