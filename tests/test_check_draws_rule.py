"""The tables of tests/check_draws_expected.py without a GPU: every entry's expected values come from the restatements of the epipolar, the
homography and the crowding rule, and this file asserts that the entries reach what tests/test_gpu_check_draws.py claims -- every outcome,
the edges of the kernels' loops, every branch of null9's pivot search (through the trace of epipolar_expected.null9) --, that deliberately
wrong restatements (the mistakes the tables exist for) change the expected bytes of at least one entry, and that the comparison functions
notice one bit, one winner and one swap.

Branches of null9 that no table entry reaches, and why:
  * a failure of kind "nonfinite".  The matrix of a hypothesis holds working coordinates |v| <= 1, their products and 1; the normal matrix of
    a refit holds sums of at most 2^31 such products.  Every step scales the remaining block so that its largest entry lies in [0.5, 1); the
    entries of the next block are a * P - b * c with all four below 1 in magnitude, so below 2.  Nothing overflows and nothing is NaN: in-range
    f32 positions cannot reach it.
  * a failure of kind "subnormal" (a largest entry whose bits are not zero and whose exponent field is).  The block before it was scaled to
    [0.5, 1), so every entry of the new block would have to fall below 2^-1022 without being zero: a * P - b * c leaves either an exact zero
    or at least half an ulp of the smaller product, and the products stay far above 2^-1022 unless entries of the scaled block are themselves
    below 2^-500.  A bounded search did not find one (COVERAGE.md, rows ext-8 and ext-9: positions 2^-e, e <= 149, on frames of 1 - 3
    columns and rows, 12 489 draws for the epipolar rule and 10 486 for the homography rule, 60 s each); tests/test_epipolar_rule.py holds
    the branch on a matrix given directly.
Everything else -- a pivot in the ninth column and in another at every step 0 .. 7, a tie for the pivot at every step, a failure at a step
<= 3 and at a later one -- is reached by both rules' tables; NULL9_REACHED below lists which combinations are asserted."""
import contextlib
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import check_draws_expected as cd
import crowd_expected as ce
import epipolar_expected as ee
import homography_expected as he
from check_draws_expected import (CONSENSUS_HYPOTHESES, CONSENSUS_LENGTHS, CONSENSUS_M_EDGES, CONSENSUS_MAX_ERRORS, CONSENSUS_SEED_VALUES, CONSENSUS_SIZES,
                                  CROWD_EDGE_NAMES, CROWD_LDS_STATES, CROWD_SEEDS, DECIDE_THREADS, FINAL_TRIP, RULES, SCORE_TRIP, SUM_TRIP, consensus_case,
                                  consensus_edge_case, consensus_edges, consensus_facts, cover_of, crowd_case, crowd_differ, crowd_edge_case, crowd_facts,
                                  crowd_grid, patched, size_classes)
from feature_draws_expected import GATHER_TILE, model_differ
from model_expected import KLT_TRACKED

CSRC = Path(__file__).resolve().parents[1] / "pyfeaturetrack_amd" / "csrc"
SEEDS = {"epipolar": cd.EPIPOLAR_SEEDS, "homography": cd.HOMOGRAPHY_SEEDS}
NULL9_REACHED = ([("pc8", k) for k in range(8)] + [("pc<8", k) for k in range(8)] + [("tie", k) for k in range(8)] + [("swap", k) for k in range(8)])


@pytest.fixture(scope="module", params=["epipolar", "homography"])
def table(request):
    """{(kind, key): case} of one rule: computed once (about 12 s a rule), shared by the tests below"""
    rule = request.param
    cases = {("edge", e["name"]): consensus_edge_case(rule, e["name"]) for e in consensus_edges(rule)}
    cases.update({("draw", s): consensus_case(rule, s) for s in SEEDS[rule]})
    return rule, cases


# ---------------------------------------------------------------------------------------------------------------- the trace hook
def _null9_before(A):
    """epipolar_expected.null9 as it stood before it took a trace, to the letter"""
    A = np.array(A, np.float64)
    perm = list(range(9))
    with np.errstate(all="ignore"):
        for k in range(8):
            best, br, bc = -1, k, k
            for i in range(k, 8):
                for j in range(k, 9):
                    b = ee._abs_bits(A[i, j])
                    if b > best:
                        best, br, bc = b, i, j
            ef = best >> 52
            if ef == 0 or ef == 0x7FF:
                return None
            A[[k, br], :] = A[[br, k], :]
            A[:, [k, bc]] = A[:, [bc, k]]
            perm[k], perm[bc] = perm[bc], perm[k]
            sc = ee._pow2(2045 - ef)
            for i in range(k, 8):
                for j in range(k, 9):
                    A[i, j] = A[i, j] * sc
            P = A[k, k]
            for i in range(k + 1, 8):
                for j in range(k + 1, 9):
                    t1 = A[i, j] * P
                    t2 = A[k, j] * A[i, k]
                    A[i, j] = t1 - t2
        x = np.zeros(9, np.float64)
        x[8] = 1.0
        for i in range(7, -1, -1):
            s = A[i, i + 1] * x[i + 1]
            for j in range(i + 2, 9):
                s = s + A[i, j] * x[j]
            for j in range(i + 1, 9):
                x[j] = x[j] * A[i, i]
            x[i] = -s
    f = np.zeros(9, np.float64)
    for c in range(9):
        f[perm[c]] = x[c]
    return f


def _rule_test_matrices():
    """the matrices of tests/test_epipolar_rule.py and tests/test_homography_rule.py that need no golden file, and rows of both rules"""
    rs = np.random.RandomState(1)
    mats = [rs.normal(size=(8, 9)) * 10.0 ** rs.randint(-3, 4) for _ in range(20)]
    A = np.random.RandomState(2).normal(size=(8, 9))
    B, C, D = A.copy(), A.copy(), A.copy()
    B[6], C[3], D[1, 4] = B[2], 0.0, np.inf
    ones = np.ones((8, 9))
    ones[np.arange(8), np.arange(8)] = -1.0
    mats += [A, B, C, D, np.full((8, 9), 5e-324), ones]
    rs = np.random.RandomState(3)
    p, q = rs.uniform(-1, 1, (2, 8)), rs.uniform(-1, 1, (2, 8))
    mats += [ee.rows_of(p[0], p[1], q[0], q[1]), he.rows_of(p[0][:4], p[1][:4], q[0][:4], q[1][:4]), he.rows_of(p[0][[0, 0, 1, 2]], p[1][[0, 0, 1, 2]],
                                                                                                              q[0][[0, 0, 1, 2]], q[1][[0, 0, 1, 2]])]
    return mats


def test_the_trace_changes_nothing_and_says_what_happened():
    assert he.null9 is ee.null9
    kinds = set()
    for A in _rule_test_matrices():
        events, called = [], []
        want, plain, traced, by_call = _null9_before(A), ee.null9(A), ee.null9(A, trace=events), ee.null9(A, trace=called.append)
        for got in (plain, traced, by_call):
            assert (got is None) == (want is None) and (want is None or got.tobytes() == want.tobytes())
        assert events == called and [e["k"] for e in events] == list(range(len(events)))
        assert (events[-1]["fail"] is not None) == (want is None) and all(e["fail"] is None for e in events[:-1])
        assert len(events) == 8 or want is None
        kinds |= {e["fail"] for e in events}
    assert kinds == {None, "zero", "subnormal", "nonfinite"}
    ones = np.ones((8, 9))
    ones[np.arange(8), np.arange(8)] = -1.0
    first = []
    ee.null9(ones, trace=first)
    assert first[0] == dict(k=0, pc8=False, tie=True, row_swap=False, col_swap=False, fail=None)
    ninth = np.random.RandomState(5).uniform(-1, 1, (8, 9))
    ninth[3, 8] = 7.0
    first = []
    ee.null9(ninth, trace=first)
    assert first[0] == dict(k=0, pc8=True, tie=False, row_swap=True, col_swap=True, fail=None)


# ---------------------------------------------------------------------------------------------------------------- consensus tables
def test_the_tables_reach_every_branch_of_null9(table):
    rule, cases = table
    cover = set()
    where = {}
    for key, c in cases.items():
        for cv in c["cover"]:
            for item in cv - cover:
                where[item] = key
            cover |= cv
    print(rule, {k: where[k] for k in sorted(where, key=str)})
    missing = [item for item in NULL9_REACHED if item not in cover]
    assert not missing, missing
    fails = sorted(item for item in cover if item[0] == "fail")
    assert {f[1] for f in fails} == {"zero"}, fails                     # (the other two kinds: the argument at the head of this file)
    assert any(f[2] <= 3 for f in fails) and any(f[2] >= 6 for f in fails), fails
    early = cases[("edge", "repeated_picks")]
    assert any(f[0] == "fail" and f[2] <= 3 for f in early["cover"][0])
    if rule == "epipolar":
        assert ("tie", 7) in cases[("edge", "integer_335")]["cover"][0]
    else:
        corners = cases[("edge", "corners")]                # a refit that takes its first pivot from the ninth column and succeeds
        assert ("pc8", 0) in corners["cover"][0] and corners["want_model"][0]["valid"] == 1 and consensus_facts(corners)[0]["flagged"] >= 1


def test_the_tables_hold_what_they_claim(table):
    rule, cases = table
    facts = {key: consensus_facts(c) for key, c in cases.items()}
    edges = {key[1]: (cases[key]["t"], f) for key, f in facts.items() if key[0] == "edge"}
    every = [(key, i, f) for key, fs in facts.items() for i, f in enumerate(fs)]
    assert len(SEEDS[rule]) == len(set(SEEDS[rule])) == 16
    assert all(len(fs) >= 2 for fs in facts.values()), "every case runs a batch"
    for key, fs in facts.items():
        assert len({f["m"] for f in fs}) == len(fs) or key == ("edge", "batch_of_every_outcome"), (key, [f["m"] for f in fs])
    # every outcome, alone and (the same lists) in a batch: 0 for each of its three reasons, 1, 2
    assert {f["valid"] for _, _, f in every} == {0, 1, 2}
    assert any(f["few"] for _, _, f in every) and any(f["singular"] for _, _, f in every) and any(f["below"] for _, _, f in every)
    few, below, fit, kept = edges["batch_of_every_outcome"][1]
    assert [f["valid"] for f in (few, below, fit, kept)] == [0, 0, 1, 2] and few["few"] and below["below"] and fit["flagged"] >= 1
    v2 = cases[("edge", "valid2")]["want_model"][0]
    # (valid 2 keeps the hypothesis, so the final pass counts the hypothesis' own inliers: n_inliers == hypothesis_inliers)
    want = dict(homography=(2, 40, 9, 25, 9), epipolar=(2, 23, 18, 19, 18))[rule]
    assert (v2["valid"], v2["n_candidates"], v2["n_inliers"], v2["hypothesis"], v2["hypothesis_inliers"]) == want
    assert np.asarray(v2["f" if rule == "epipolar" else "h"]).any(), "valid 2 publishes the hypothesis"
    assert edges["valid2"][1][0]["flagged"] >= 1 and edges["one_point"][1][0]["singular"]
    # candidate counts on the edges of the three loops: a model that keeps and flags candidates in the last partial trip of every loop --
    # a trip of one candidate (m = 257, 513: an inlier, which the score and the sums lose with it; m = 2049: a flagged one, which the
    # final pass loses with it) cannot hold both
    assert CONSENSUS_M_EDGES == [255, 256, 257, 511, 512, 513, 2047, 2048, 2049] and (SCORE_TRIP, SUM_TRIP, FINAL_TRIP) == (256, 512, 2048)
    for m in CONSENSUS_M_EDGES:
        f = edges["m%d" % m][1][0]
        assert f["m"] == m and f["valid"] == 1 and f["flagged"] >= 1 and f["kept"] >= 1
        for trip in (SCORE_TRIP, SUM_TRIP, FINAL_TRIP):
            tail = f["tails"][trip]
            assert (tail is None) == (m % trip == 0)
            if tail is not None and m % trip > 1:
                assert tail[0] >= 1 and tail[1] >= 1, (m, trip, tail)
    assert edges["m257"][1][0]["tails"][SCORE_TRIP] == (1, 0) and edges["m513"][1][0]["tails"][SUM_TRIP] == (1, 0)
    assert edges["m2049"][1][0]["tails"][FINAL_TRIP] == (0, 1)
    # list lengths around one and two tiles of the gather; more than one pair of a batch above a tile
    for n in CONSENSUS_LENGTHS:
        t, fs = edges["n%d" % n]
        assert t["n"] == n and all(f["valid"] == 1 and f["flagged"] >= 1 for f in fs)
        assert [len(f["tile_candidates"]) for f in fs] == [(n + GATHER_TILE - 1) // GATHER_TILE] * 2 and all(min(f["tile_candidates"]) >= 1 for f in fs)
    assert any(len(f["tile_candidates"]) == 2 for key, _, f in every if key[0] == "draw")
    # hypothesis counts; a best hypothesis the first pass of the strided argmax does not see; ties won by neither the first nor the last
    assert CONSENSUS_HYPOTHESES == [1, 4, 5, 511, 512, 513, 1001, 4096] and DECIDE_THREADS == 512
    assert {cases[key]["t"]["params"]["hypotheses"] for key in cases} >= set(CONSENSUS_HYPOTHESES)
    assert all(edges["h%d" % h][0]["params"]["hypotheses"] == h for h in CONSENSUS_HYPOTHESES)
    late = [(key, i, f["best"]) for key, i, f in every if f["best"] >= DECIDE_THREADS]
    assert any(i == 0 for _, i, _ in late) and len({key for key, _, _ in late}) >= 2, late
    assert any(f["best"] >= 2 * DECIDE_THREADS for _, _, f in every)                  # (the third pass and later)
    ties = [(key, f["best"]) for key, _, f in every if f["tie"] and 0 < f["best"] < cases[key]["t"]["params"]["hypotheses"] - 1]
    assert ties, "no tie for the top score is won by a hypothesis that is neither the first nor the last"
    for key, i, f in every:
        scores = cases[key]["scores"][i]
        if f["tie"]:
            assert f["best"] == int(np.flatnonzero(scores == scores.max())[0])
    # seeds, sizes, thresholds
    seeds = {cases[key]["t"]["params"]["seed"] for key in cases}
    assert seeds >= set(CONSENSUS_SEED_VALUES) and CONSENSUS_SEED_VALUES == [0, 1, 0x7fffffff, 0x80000000, 0xffffffff, 0x9e3779b9]
    assert any(s >= 1 << 31 and s not in CONSENSUS_SEED_VALUES for s in seeds)
    sizes = {(cases[key]["t"]["ncols"], cases[key]["t"]["nrows"]) for key in cases}
    assert sizes >= set(CONSENSUS_SIZES)
    classes = set().union(*(size_classes(*s) for s in sizes))
    assert classes >= {"tall", "wide", "square", "power_of_two", "power_of_two_plus_1", "tiny", "bit31"}
    for size in CONSENSUS_SIZES:
        t, fs = edges["size_%dx%d" % size]
        assert fs[0]["valid"] == 1 and (int(cases[("edge", "size_%dx%d" % size)]["want_model"][0]["pad"]) < 0) == (size[1] >= 32768)
    assert any("bit31" in size_classes(*s) for s in {(cases[k]["t"]["ncols"], cases[k]["t"]["nrows"]) for k in cases if k[0] == "draw"})
    c = cases[("edge", "size_512x512")]
    assert ee.scale_of(512, 512) == 2.0 ** -8 and c["pairs"][0]["x"][1] == 0 and c["pairs"][0]["y"][2] == 0 and c["pairs"][1]["x"][3] == 0
    px, py, qx, qy = ee.working(c["pairs"][0], c["pairs"][1], np.arange(300) < 5, 512, 512)
    assert px[1] == -1.0 and py[2] == -1.0 and qx[3] == -1.0 and qy[4] == -1.0          # working coordinates of exactly -1
    assert ee.scale_of(256, 256) == 2 * ee.scale_of(257, 200) == 2 * ee.scale_of(200, 257)        # either side of a change of k
    assert {np.float32(e) for e in CONSENSUS_MAX_ERRORS} <= {np.float32(cases[key]["t"]["params"]["max_error"]) for key in cases}
    assert all(edges["max_error_%g" % e][0]["params"]["max_error"] == e for e in CONSENSUS_MAX_ERRORS)
    # every kind of non-candidate in every draw and in the scene lists of the edges
    from model_expected import candidate_mask
    for key, c in cases.items():
        t = c["t"]
        if key[0] == "draw" or key[1][0] in "mnhs":
            cand = candidate_mask(c["pairs"][0], c["pairs"][1], t["ncols"], t["nrows"])
            assert (~cand).sum() >= 35 or t["n"] < 40, key
    for key, i, f in every:
        if f["valid"] == 0:
            assert f["flagged"] == 0 and f["best"] == -1 and cases[key]["want_out"][i].tobytes() == cases[key]["pairs"][2 * i + 1].tobytes()


def test_the_kernels_constants_are_the_sources():
    """the trips, the stride, the gather's tile, the LDS threshold and the grid rule that the tables are built around, as the sources spell them"""
    text = (CSRC / "consensus_primitives.h").read_text()
    ahead = re.search(r"constexpr int SCORE_AHEAD = (\d+), SUM_AHEAD = (\d+), FINAL_AHEAD = (\d+);", text)
    threads = int(re.search(r"constexpr int DECIDE_THREADS = (\d+);", text).group(1))
    assert (64 * int(ahead.group(1)), 64 * int(ahead.group(2)), threads * int(ahead.group(3))) == (SCORE_TRIP, SUM_TRIP, FINAL_TRIP)
    assert threads == DECIDE_THREADS and "for (int h = t; h < hypotheses; h += THREADS)" in text
    assert "k0 += 64 * SCORE_AHEAD" in text and "k0 += THREADS * FINAL_AHEAD" in text
    assert int(re.search(r"constexpr int kCrowdLdsStates = (\d+);", (CSRC / "klt_internal.h").read_text()).group(1)) == CROWD_LDS_STATES
    kernels = (CSRC / "crowd_kernels.hip").read_text()
    assert int(re.search(r"constexpr int RESOLVE_THREADS = (\d+);", kernels).group(1)) == cd.CROWD_SCAN_LANES
    assert "const int per = (ncells + RESOLVE_THREADS - 1) / RESOLVE_THREADS;" in kernels and "if (a.n <= kCrowdLdsStates)" in kernels
    api = (CSRC / "api_crowd.hip").read_text()
    body = api[api.index("static void fill_crowd_grid"):api.index("static size_t crowd_slice_bytes")]
    assert "a.r = p.min_distance - 1;" in body and "side = p.min_distance > %d ? p.min_distance : %d;" % (cd.CROWD_MIN_SIDE, cd.CROWD_MIN_SIDE) in body
    assert "if ((long long)a.gx * a.gy <= %d) break;" % cd.CROWD_MAX_CELLS in body and "side *= 2;" in body
    assert "a.gx = (int)((p.ncols + side - 1) / side); a.gy = (int)((p.nrows + side - 1) / side);" in body
    assert crowd_grid(4096, 4096, 10) == (16, 256, 256) and crowd_grid(4097, 4096, 10) == (32, 129, 128) and crowd_grid(4096, 4097, 10) == (32, 128, 129)
    assert crowd_grid(65535, 65535, 10) == (256, 256, 256) and crowd_grid(320, 240, 17) == (17, 19, 15)
    assert crowd_grid(320, 240, 65536) == (65536, 1, 1) and crowd_grid(320, 240, 0x7fffffff) == (0x7fffffff, 1, 1)
    assert crowd_grid(65535, 65535, 300) == (300, 219, 219) and crowd_grid(65535, 65535, 200)[0] == 400


# ---------------------------------------------------------------------------------------------------------------- consensus mutants
def _recompiled(fn, *edits, **names):
    """`fn` compiled again from its source with `edits` = (old, new) applied, each exactly once, in its module's namespace plus `names`"""
    src = inspect.getsource(fn)
    for old, new in edits:
        assert src.count(old) == 1, "%s has changed: %r stands in it %d times" % (fn.__name__, old, src.count(old))
        src = src.replace(old, new)
    ns = dict(vars(inspect.getmodule(fn)), **names)
    exec(compile(src, "<a wrong %s>" % fn.__name__, "exec"), ns)
    return ns[fn.__name__]


def _null9_patch(*edits):
    wrong = _recompiled(ee.null9, *edits)
    return [(ee, dict(null9=wrong)), (he, dict(null9=wrong))]


def _expected_patch(rule, *edits, **names):
    fn = getattr(RULES[rule].mod, RULES[rule].expected)
    return [(RULES[rule].mod, {RULES[rule].expected: _recompiled(fn, *edits, **names)})]


def _drop_tail(mod, trip):
    original = mod.inliers

    def inliers(f, px, py, qx, qy, t2):
        r = np.array(original(f, px, py, qx, qy, t2))
        r[len(r) - len(r) % trip:] = False
        return r
    return [(mod, dict(inliers=inliers))]


def _sequential_sums():
    def _sum64(terms, inl):
        s = np.float64(0.0)
        for v in np.asarray(terms)[np.asarray(inl, bool)]:
            s = s + v
        return s
    return [(ee, dict(_sum64=_sum64)), (he, dict(_sum64=_sum64))]


def _sign_extended_seed(rule):
    from model_expected import mix, mulhi32
    picks_per = RULES[rule].picks

    def hashed(seed, v):
        x = (seed | 0xFFFFFFFF00000000 if seed & 0x80000000 else seed) ^ mix(v)       # the xor and the first shift in 64 bits
        x ^= x >> 16
        x = ((x & 0xFFFFFFFF) * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)

    def picks(seed, h, m):
        return tuple(mulhi32(hashed(seed & 0xFFFFFFFF, (picks_per * h + j) & 0xFFFFFFFF), m) for j in range(picks_per))
    return [(RULES[rule].mod, dict(picks=picks))]


def _padding_counted(model, t2, m, mod):
    """the candidates (0, 0, 0, 0) up to the next multiple of the final loop's trip, where the model takes them for inliers"""
    z = np.zeros(1, np.float64)
    with np.errstate(all="ignore"):
        return (-m % FINAL_TRIP) * int(mod.inliers(model, z, z, z, z, t2)[0])


def consensus_mutants(rule):
    """name -> (patches, the entries it must change at least one of)"""
    mod = RULES[rule].mod
    best_line = "    best = int(np.argmax(scores))                   # the first of the largest: ties go to the smallest h\n"
    free = _recompiled(ee.free_index, ("abs(f[i]) > abs(f[g])", "abs(f[i]) >= abs(f[g])"))
    from model_expected import mix, mulhi32
    m = {
        "pivot ties go to the last position": (_null9_patch(("if b > best:", "if b >= best:")), ["valid2", "batch_of_every_outcome", "size_5x3"]),
        "the permutation forgets a pivot in the ninth column": (_null9_patch(("            perm[k], perm[bc] = perm[bc], perm[k]\n",
                                                                              "            if bc != 8: perm[k], perm[bc] = perm[bc], perm[k]\n")), ["m255", "valid2"]),
        "argmax over the first 512 hypotheses only": (_expected_patch(rule, (best_line, "    best = int(np.argmax(scores[:512]))\n")), ["h1001"]),
        "score ties go to the largest h": (_expected_patch(rule, (best_line, "    best = len(scores) - 1 - int(np.argmax(scores[::-1]))\n")), ["m255", "size_5x3"]),
        "the free index ties to the largest": ([(ee, dict(free_index=free)), (he, dict(free_index=free))],
                                               ["integer_1674", "valid2", "batch_of_every_outcome"]),
        "padding candidates counted": (_expected_patch(rule, ("int(final.sum()), best", "int(final.sum()) + _pad(model, t2, m, _mod), best"),
                                                       _pad=_padding_counted, _mod=mod), ["size_5x3", "m255", "m2049"]),
        "candidates past the last full trip dropped": (_drop_tail(mod, SCORE_TRIP), ["m257", "m513"]),
        "sums added one after the other": (_sequential_sums(), ["seed_00000000", "m513"]),
        "valid 2 publishes zeros": (_expected_patch(rule, ("else (hyp, 2)", "else (np.zeros(9, np.float64), 2)")), ["valid2"]),
        "s from ncols alone": ([(ee, dict(scale_of=lambda ncols, nrows, _f=ee.scale_of: _f(ncols, ncols)))], ["size_200x257", "size_640x40000"]),
        "the seed sign-extended": (_sign_extended_seed(rule), ["seed_80000000", "seed_ffffffff", "seed_9e3779b9"]),
    }
    if rule == "homography":
        m["the permutation forgets a pivot in the ninth column at step 0"] = (_null9_patch(
            ("            perm[k], perm[bc] = perm[bc], perm[k]\n", "            if bc != 8 or k: perm[k], perm[bc] = perm[bc], perm[k]\n")), ["corners"])
        m["eight picks a hypothesis"] = ([(he, dict(picks=lambda seed, h, n: tuple(mulhi32(mix((seed & 0xFFFFFFFF) ^ mix((8 * h + j) & 0xFFFFFFFF)), n)
                                                                                     for j in range(4))))], ["seed_00000000"])
    return m


def _changed(rule, patches, names):
    """the entries among `names` whose expected bytes a wrong restatement changes"""
    cases = {name: consensus_edge_case(rule, name) for name in names if name in [e["name"] for e in consensus_edges(rule)]}      # (before the patch)
    changed = []
    with contextlib.ExitStack() as stack:
        for mod, repl in patches:
            stack.enter_context(patched(mod, **repl))
        fn = getattr(RULES[rule].mod, RULES[rule].expected)
        for name, c in cases.items():
            t = c["t"]
            for i in range(len(c["want_out"])):
                out, model = fn(c["pairs"][2 * i], c["pairs"][2 * i + 1], t["ncols"], t["nrows"], **t["params"])
                if model_differ(out, model, c["want_out"][i], c["want_model"][i], name, RULES[rule].dtype) is not None:
                    changed.append(name)
                    break
    return changed


@pytest.mark.parametrize("rule", ["epipolar", "homography"])
def test_wrong_restatements_change_a_table_entry(rule):
    """the mistakes the tables exist for, each as a wrong copy of the restatement: at least one entry's expected bytes change"""
    unseen = []
    for what, (patches, names) in consensus_mutants(rule).items():
        changed = _changed(rule, patches, names)
        print("%s: %s -> %r" % (rule, what, changed))
        if not changed:
            unseen.append(what)
    assert not unseen, unseen
    assert _changed(rule, [], ["m255", "valid2", "seed_80000000"]) == []           # (and the right one changes none)
    for name in ("seed_00000000", "seed_00000001", "seed_7fffffff"):                # a seed below 2^31 is the same number sign-extended
        assert _changed(rule, _sign_extended_seed(rule), [name]) == []


# ---------------------------------------------------------------------------------------------------------------- crowding
@pytest.fixture(scope="module")
def crowd_table():
    cases = {("edge", name): crowd_edge_case(name) for name in CROWD_EDGE_NAMES}
    cases.update({("draw", s): crowd_case(s) for s in CROWD_SEEDS})
    return cases


def test_the_crowd_tables_hold_what_they_claim(crowd_table):
    facts = {key: crowd_facts(c) for key, c in crowd_table.items()}
    edges = {key[1]: f for key, f in facts.items() if key[0] == "edge"}
    assert len(CROWD_SEEDS) == len(set(CROWD_SEEDS)) == 12
    # the cell-count boundary: 65 536 cells of 16 pixels; a cell column or row more doubles the side; the largest frame
    assert (edges["cells_4096x4096"]["side"], edges["cells_4096x4096"]["ncells"]) == (16, 65536)
    assert edges["cells_4097x4096"]["side"] == edges["cells_4096x4097"]["side"] == 32 and edges["cells_65535x65535"]["side"] == 256
    for name in ("cells_4096x4096", "cells_4097x4096", "cells_4096x4097", "cells_65535x65535", "d17"):
        c, f = crowd_table[("edge", name)], edges[name]
        out, crowd = c["outs"][0], c["want_crowd"][0]
        assert 200 <= len(out) <= 400 and f["crowded"][0] >= 40 and f["kept"][0] >= 100
        px, py = out["x"].astype(np.int64), out["y"].astype(np.int64)
        r = c["t"]["d"] - 1
        across = {"x": 0, "y": 0, "xy": 0}
        for i in range(14, len(out) - 1, 2):                 # (behind border_pairs' fourteen records: the drawn pairs, two records each)
            j = i + 1
            dx, dy = abs(int(px[i] - px[j])), abs(int(py[i] - py[j]))
            cx, cy = px[i] // f["side"] != px[j] // f["side"], py[i] // f["side"] != py[j] // f["side"]
            if max(dx, dy) in (r, r + 1) and (cx or cy):
                across["xy" if cx and cy else "x" if cx else "y"] += 1
        assert min(across.values()) >= 10, (name, across)                          # pairs r and r + 1 apart across a border in x, in y, diagonally
        assert (px // f["side"]).max() == f["gx"] - 1 or (py // f["side"]).max() == f["gy"] - 1 or name == "d17"
    assert edges["d17"]["side"] == 17
    for name in ("d65536", "d_int32_max"):
        assert edges[name]["ncells"] == 1 and edges[name]["kept"][0] == 1 and edges[name]["crowded"][0] == edges[name]["candidates"][0] - 1
    assert (edges["one_cell_row"]["gy"], edges["one_cell_column"]["gx"]) == (1, 1) and edges["one_cell_row"]["gx"] > 300 < edges["one_cell_column"]["gy"]
    for k in (1, 1023, 1024, 1025, 2049):
        assert edges["ncells_%d" % k]["ncells"] == k and edges["ncells_%d" % k]["side"] == 16 and edges["ncells_%d" % k]["crowded"][0] >= 1
    assert {f["scan"] for f in facts.values()} == {"one cell", "fewer cells than lanes", "a cell a lane", "2 cells a lane, lanes idle", "3 cells and more a lane",
                                                    "64 cells a lane, all full"}
    sides = {f["side"] for f in facts.values()}
    assert sides >= {16, 17, 32, 256, 65536, 0x7fffffff} and any(f["side"] == crowd_table[k]["t"]["d"] > 17 for k, f in facts.items())
    for name, n in (("n1_on_4k", 1), ("n3_on_4k", 3)):
        assert crowd_table[("edge", name)]["t"]["n"] == n and edges[name]["ncells"] == 240 * 135 > 256 * n
    assert edges["n3_on_4k"]["crowded"][0] == 1
    # the resolve kernel without LDS states, single and in a batch (the launch is sized by the common n)
    for name in ("batch_above_lds", "batch_across_lds", "chain_in_scratch"):
        assert crowd_table[("edge", name)]["t"]["n"] == CROWD_LDS_STATES + 1 and not edges[name]["lds"] and len(crowd_table[("edge", name)]["outs"]) >= 2
        assert min(edges[name]["crowded"]) >= 1000 and min(edges[name]["kept"]) >= 1000
    assert edges["batch_above_lds"]["candidates"][0] == CROWD_LDS_STATES + 1 and edges["batch_across_lds"]["candidates"][0] == CROWD_LDS_STATES + 1
    assert edges["batch_across_lds"]["candidates"][1] == CROWD_LDS_STATES         # (the launch goes by n, not by the candidates)
    assert any(f["lds"] for f in facts.values())
    c = crowd_table[("edge", "chain_in_scratch")]
    assert c["want_crowd"][0]["val"][:cd.CROWD_CHAIN].tolist().count(2) >= cd.CROWD_CHAIN // 2 - 2             # the chain alternates kept / crowded
    px, py, order = _walk_inputs(c["outs"][0][:cd.CROWD_CHAIN], c["prevs"][0][:cd.CROWD_CHAIN], 3000, 300)
    assert ce.parallel_rounds(px, py, order, 9)[1] == cd.CROWD_CHAIN
    ages = crowd_table[("edge", "age_extremes")]["prevs"][0]["age"]
    assert {ce.INT32_MAX, ce.INT32_MAX - 1} <= set(ages.tolist()) and (ages < 0).sum() >= 3
    got = crowd_table[("edge", "age_extremes")]["want_crowd"][0]
    assert (got["age"] == ce.INT32_MAX).sum() >= 2
    assert any(crowd_table[k]["t"].get("ages") for k in crowd_table if k[0] == "draw")
    for key, c in crowd_table.items():                       # every list of a case holds another number of candidates; non-candidates of every kind
        f = facts[key]
        assert len(set(f["candidates"])) == len(f["candidates"]) or c["t"]["n"] <= 3, (key, f["candidates"])
        if key[0] == "draw":
            assert c["t"]["n"] - f["candidates"][0] >= 20


def _walk_inputs(out, prev, ncols, nrows):
    cand = ce.candidate_mask(out, ncols, nrows)
    px, py = ce.pixels(out, cand)
    return px, py, ce.priority_order(cand, ce.ages_in(prev, len(out)))


def crowd_mutants():
    """name -> (patches of crowd_expected, the entries it must change at least one of)"""
    def higher_index(cand, age):
        idx = np.flatnonzero(cand)
        return idx[np.lexsort((-idx, -age[idx]))]

    def unclamped(prev, n):
        return np.zeros(n, np.int64) if prev is None else np.asarray(prev["age"], np.int64)

    def rounded(out, cand):
        px, py = np.zeros(len(out), np.int64), np.zeros(len(out), np.int64)
        px[cand], py[cand] = np.floor(out["x"][cand].astype(np.float64) + 0.5).astype(np.int64), np.floor(out["y"][cand].astype(np.float64) + 0.5).astype(np.int64)
        return px, py
    any_winner = _recompiled(ce.serial_walk, ("int(kept[np.argmax(covering)])", "int(kept[len(covering) - 1 - np.argmax(covering[::-1])])"))
    own_cell = {side: _recompiled(ce.serial_walk, ("(np.abs(ky[:nk] - py[i]) <= r)", "(np.abs(ky[:nk] - py[i]) <= r) & (kx[:nk] // _side == px[i] // _side) "
                                                                                        "& (ky[:nk] // _side == py[i] // _side)"), _side=side) for side in (16, 17, 32)}
    wider = _recompiled(ce.crowd_check_expected, ("n, r = len(out), min_distance - 1", "n, r = len(out), min_distance"))
    wrapping = _recompiled(ce.crowd_check_expected, ("min(int(age[i]), INT32_MAX - 1) + 1", "(int(age[i]) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31"))
    return {
        "equal ages favour the higher index": ([dict(priority_order=higher_index)], ["ncells_1024"]),
        "negative ages not clamped": ([dict(ages_in=unclamped)], ["age_extremes"]),
        "the winner is any covering kept candidate": ([dict(serial_walk=any_winner)], ["ncells_1", "batch_above_lds"]),
        "neighbours in the candidate's own cell only": ([dict(serial_walk=own_cell[16])], ["cells_4096x4096", "ncells_1024"]),
        "own cell only, side 17": ([dict(serial_walk=own_cell[17])], ["d17"]),
        "own cell only, side 32": ([dict(serial_walk=own_cell[32])], ["cells_4097x4096", "cells_4096x4097"]),
        "r = d": ([dict(crowd_check_expected=wider)], ["cells_4096x4096", "d17"]),
        "pixels by rounding": ([dict(pixels=rounded)], ["ncells_1024", "d17"]),
        "no saturation at INT32_MAX": ([dict(crowd_check_expected=wrapping)], ["age_extremes"]),
    }


def test_wrong_crowding_rules_change_a_table_entry(crowd_table):
    unseen = []
    for what, (patches, names) in crowd_mutants().items():
        changed = []
        with contextlib.ExitStack() as stack:
            for repl in patches:
                stack.enter_context(patched(ce, **repl))
            for name in names:
                c = crowd_table[("edge", name)]
                t = c["t"]
                out, crowd = ce.crowd_check_expected(c["outs"][0], c["prevs"][0], t["ncols"], t["nrows"], t["d"])
                if crowd_differ(out, crowd, c["want_out"][0], c["want_crowd"][0], name) is not None:
                    changed.append(name)
        print("%s -> %r" % (what, changed))
        if not changed:
            unseen.append(what)
    assert not unseen, unseen


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def test_the_comparisons_notice_one_bit_one_winner_and_one_swap(crowd_table):
    for rule in ("epipolar", "homography"):
        c = consensus_edge_case(rule, "m2049")
        out, model, dtype = c["want_out"][0], c["want_model"][0], RULES[rule].dtype
        kept = np.flatnonzero(out["val"] == KLT_TRACKED)
        assert model_differ(out.copy(), model.copy(), out, model, "same", dtype) is None
        coef = dtype.names[0]
        for k in range(9):
            rec = np.array(model)
            rec[coef].view(np.int64)[k] ^= 1                 # one low mantissa bit of one coefficient
            assert model_differ(out, rec, out, model, "bit", dtype) is not None, (rule, k)
        for field in ("valid", "n_candidates", "n_inliers", "hypothesis", "hypothesis_inliers", "pad"):
            rec = np.array(model)
            rec[field] += 1
            assert model_differ(out, rec, out, model, field, dtype) is not None
        flip = out.copy()
        flip["x"].view(np.int32)[kept[-1]] ^= 1
        assert model_differ(flip, model, out, model, "flip", dtype) is not None
        swap = out.copy()
        swap[[kept[0], kept[-1]]] = swap[[kept[-1], kept[0]]]
        assert model_differ(swap, model, out, model, "swap", dtype) is not None
        assert model_differ(out[:-1], model, out, model, "short", dtype) is not None
    c = crowd_table[("edge", "ncells_1024")]
    out, crowd = c["want_out"][0], c["want_crowd"][0]
    assert crowd_differ(out.copy(), crowd.copy(), out, crowd, "same") is None
    lost = np.flatnonzero(crowd["val"] == 2)
    wrong = crowd.copy()
    wrong["winner"][lost[0]] += 1
    assert crowd_differ(out, wrong, out, crowd, "winner") is not None
    wrong = crowd.copy()
    wrong["age"][np.flatnonzero(crowd["val"] == 1)[0]] ^= 1
    assert crowd_differ(out, wrong, out, crowd, "age") is not None
    kept = np.flatnonzero(crowd["val"] == 1)
    swap = out.copy()
    swap[[kept[0], kept[1]]] = swap[[kept[1], kept[0]]]
    assert crowd_differ(swap, crowd, out, crowd, "swap") is not None
    swap = crowd.copy()
    swap[[kept[0], lost[0]]] = swap[[lost[0], kept[0]]]
    assert crowd_differ(out, swap, out, crowd, "swapped crowd records") is not None
    zero = out.copy()
    zero["x"][kept[0]] = -0.0 if out["x"][kept[0]] == 0 else out["x"][kept[0]]
    flip = out.copy()
    flip["y"].view(np.int32)[kept[0]] ^= 1
    assert crowd_differ(flip, crowd, out, crowd, "flip") is not None
    assert cover_of([dict(k=2, pc8=True, tie=True, row_swap=False, col_swap=True, fail=None), dict(k=3, pc8=False, tie=True, row_swap=False, col_swap=False,
                                                                                                  fail="zero")]) == {("pc8", 2), ("tie", 2), ("swap", 2), ("fail", "zero", 3)}
