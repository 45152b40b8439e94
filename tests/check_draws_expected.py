"""TEST INFRASTRUCTURE ONLY -- seeded draws and fixed edge tables for the epipolar check, the homography check (DESIGN.md sections 9h, 9i;
one score_kernel / decide_kernel pair in csrc/consensus_primitives.h) and the crowding check (section 9j), and the trial functions that
run one table entry on a device context.  Expected values are the restatements' (tests/epipolar_expected.py, homography_expected.py,
crowd_expected.py), compared byte for byte.  tests/test_check_draws_rule.py asserts without a GPU that the tables reach what they claim;
tests/test_gpu_check_draws.py runs them; tests/fuzz/fuzz_parity.py --epipolar / --homography / --crowd runs fresh draws."""
import collections
import contextlib
import functools

import numpy as np

import crowd_expected as ce
import epipolar_expected as ee
import homography_expected as he
from feature_draws_expected import GATHER_TILE, MODEL_HYPOTHESES, MODEL_M_EDGES, MODEL_MAX_ERRORS, _readonly, _thin, model_differ
from model_expected import FEAT_DTYPE, KLT_TRACKED, candidate_mask, non_candidate_kinds, records

# ------------------------------------------------------------------------------------------------------- what the kernels' loops take
SCORE_TRIP, SUM_TRIP, FINAL_TRIP = 256, 512, 2048       # candidates per trip: count_inliers (64 x SCORE_AHEAD), add_sums (64 x SUM_AHEAD),
DECIDE_THREADS = 512                                    # flag_outliers (512 x FINAL_AHEAD); the stride of reduce_best_key
CROWD_LDS_STATES = 24576                                # kCrowdLdsStates
CROWD_SCAN_LANES = 1024                                 # RESOLVE_THREADS: every lane scans ceil(ncells / 1024) cells
CROWD_MIN_SIDE, CROWD_MAX_CELLS = 16, 65536             # fill_crowd_grid

Rule = collections.namedtuple("Rule", "name mod expected dtype outlier scene picks min_inliers matrix")
RULES = {
    "epipolar": Rule("epipolar", ee, "epipolar_check_expected", ee.EPIPOLAR_DTYPE, ee.KLT_EPIPOLAR_OUTLIER, ee.parallax_n, 8, 8, ee.epipolar_matrix),
    "homography": Rule("homography", he, "homography_check_expected", he.HOMOGRAPHY_DTYPE, he.KLT_HOMOGRAPHY_OUTLIER, he.rotation_n, 4, 4,
                       he.homography_matrix),
}
CONSENSUS_HYPOTHESES = MODEL_HYPOTHESES                 # 1, 4, 5, 511, 512, 513, 1001, 4096
CONSENSUS_MAX_ERRORS = MODEL_MAX_ERRORS                 # 0.0, 0.01, 0.5, 1.0, 3.0
CONSENSUS_M_EDGES = MODEL_M_EDGES                       # 255 ... 2049
CONSENSUS_SEED_VALUES = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff, 0x9e3779b9]
CONSENSUS_LENGTHS = [8191, 8192, 8193, 16385]
CONSENSUS_SIZES = [(4, 4), (5, 3), (256, 256), (257, 200), (200, 257), (512, 512), (640, 40000), (65535, 65535), (32768, 32769)]
SCENE_SIZE = (1920, 1080)                               # the scenes are drawn on this frame and scaled to the case's


def size_classes(ncols, nrows):
    """the classes of a frame size the working scale s = 2^-k and the record's size word care about"""
    big = max(ncols, nrows)
    cls = {"tall" if nrows > ncols else "wide" if ncols > nrows else "square"}
    if big & (big - 1) == 0:
        cls.add("power_of_two")
    if (big - 1) & (big - 2) == 0 and big > 2:
        cls.add("power_of_two_plus_1")
    if big <= 8:
        cls.add("tiny")
    if nrows >= 32768:
        cls.add("bit31")
    return cls


# ------------------------------------------------------------------------------------------------------------------- consensus lists
def scene_lists(rule, n, ncols, nrows, seed, kinds=None):
    """n records of the rule's smooth scene (parallax_n / rotation_n on 1920 x 1080, a tenth of them displaced), scaled to the frame --
    positions inside it, the motion and the noise scaled with it --, in a drawn order, so that the displaced records stand anywhere among
    the candidates; `kinds` = (start, step): every kind of non-candidate spread over the list"""
    fin, fout, _ = rule.scene(n, SCENE_SIZE[0], SCENE_SIZE[1], seed)
    if (ncols, nrows) != SCENE_SIZE:
        sx, sy = ncols / float(SCENE_SIZE[0]), nrows / float(SCENE_SIZE[1])
        for fl in (fin, fout):
            fl["x"] = fl["x"].astype(np.float64) * sx
            fl["y"] = fl["y"].astype(np.float64) * sy
    order = np.random.default_rng([seed, 21]).permutation(n)
    fin, fout = fin[order].copy(), fout[order].copy()
    assert candidate_mask(fin, fout, ncols, nrows).all()
    if kinds is not None:
        non_candidate_kinds(fin, fout, ncols, nrows, start=kinds[0], step=kinds[1])
    return fin, fout


def integer_lists(trial, n=None):
    """integer positions on a 64 x 64 frame under an integer translation, +-1 added to qx of about a fifth of the records in half of the
    draws; either all drawn apart or 2 - 9 points repeated: every product of the rules is exact, so models exist under max_error 0"""
    rng = np.random.default_rng([trial, 7])
    drawn = int(rng.integers(8, 41))
    n = drawn if n is None else n
    if rng.random() < 0.5:
        k = int(rng.integers(2, 10))
        bx, by = rng.integers(0, 64, k), rng.integers(0, 64, k)
        idx = np.arange(n) % k
        x, y = bx[idx], by[idx]
    else:
        x, y = rng.integers(0, 64, n), rng.integers(0, 64, n)
    tx, ty = rng.integers(-2, 3, 2)
    qx, qy = x + tx, y + ty
    if rng.random() < 0.5:
        qx = qx + np.where(rng.random(n) < 0.2, rng.choice([-1, 1], n), 0)
    return records(x, y, 1), records(qx, qy)


def valid2_lists(rule_name):
    """an input whose refit fails (an exactly zero block in null9 of the normal matrix): valid == 2, the hypothesis is kept"""
    if rule_name == "homography":
        x, y = np.array([39, 57, 57, 19] * 10), np.array([18, 61, 63, 38] * 10)
        qx, qy = x - 1, y - 1
        qx[[5, 11, 14, 27]] = [55, 19, 57, 17]
    else:
        x = np.array([1, 3, 57, 15, 20, 14, 36, 46, 9, 7, 46, 3, 55, 9, 13, 12, 31, 58, 38, 11, 34, 13, 29, 7])
        y = np.array([1, 43, 53, 13, 63, 13, 58, 47, 0, 51, 7, 19, 53, 61, 32, 51, 34, 36, 2, 39, 34, 20, 2, 8])
        qx, qy = x - 1, y - 1                       # (record 8: qy = -1, no candidate)
        qx[13] = 7
    return records(x, y, 1), records(qx, qy)


VALID2_PARAMS = {"homography": dict(hypotheses=64, seed=76, min_inliers=4, max_error=0.0),
                 "epipolar": dict(hypotheses=64, seed=945, min_inliers=8, max_error=0.0)}
VALID2_SIZE = (64, 64)


def _padded(fin, fout, n):
    """the lists with non-candidates behind them (lost in `out`, positions off the frame), n records in all"""
    k = n - len(fin)
    assert k >= 0
    return np.concatenate([fin, records(np.full(k, -1.0), np.full(k, -1.0), -1)]), np.concatenate([fout, records(np.full(k, -1.0), np.full(k, -1.0), -3)])


def consensus_every_outcome_batch(rule_name):
    """four pairs under the parameters of the valid-2 list: too few candidates; candidates without a consensus (random positions, no two
    alike under max_error 0); an exact integer translation with a few records off it (a refit: valid 1, records flagged); the valid-2 list"""
    rule = RULES[rule_name]
    ncols, nrows = VALID2_SIZE
    n = 48
    rs = np.random.RandomState(9)
    fit = integer_lists(0)
    few = tuple(fl[:rule.min_inliers - 1] for fl in fit)
    none = (records(rs.uniform(1, 62, 40), rs.uniform(1, 62, 40), 1), records(rs.uniform(1, 62, 40), rs.uniform(1, 62, 40)))
    pairs = [_padded(*p, n) for p in (few, none, fit, valid2_lists(rule_name))]
    return dict(name="batch_of_every_outcome", n=n, ncols=ncols, nrows=nrows, params=dict(VALID2_PARAMS[rule_name])), pairs


def _cedge(name, n, size=SCENE_SIZE, m=None, params=None, list_seed=None, **more):
    return dict(dict(name=name, n=n, ncols=size[0], nrows=size[1], m=m, list_seed=list_seed if list_seed is not None else 2000 + n,
                     params=dict(dict(hypotheses=64, seed=0x9e3779b9, min_inliers=8, max_error=0.5), **(params or {}))), **more)


def _size_error(size, unscaled=(5, 3)):
    """max_error for a frame of this size: half a pixel of the scene's frame, scaled as the scene is (the 5 x 3 frame keeps 0.5 px, under
    which every candidate and the padding candidate (0, 0, 0, 0) are inliers)"""
    return 0.5 if size == unscaled else float(np.float32(0.5 * max(size[0] / float(SCENE_SIZE[0]), size[1] / float(SCENE_SIZE[1]))))


def consensus_edges(rule_name):
    """the fixed cases of a rule beside its draws"""
    rule = RULES[rule_name]
    lo = rule.min_inliers
    edges = [_cedge("m%d" % m, m + 150 + m // 8, m=m) for m in CONSENSUS_M_EDGES]
    edges += [_cedge("n%d" % n, n) for n in CONSENSUS_LENGTHS]
    # a threshold of 0.15 px on 0.1 px of noise: the scores differ from hypothesis to hypothesis, the best one stands anywhere
    # (4096 hypotheses: the list that shares the batch has too few candidates, so that the restatement runs null9 4096 times, not 8192)
    edges += [_cedge("h%d" % h, 300, params=dict(hypotheses=h, max_error=0.15 if h > 5 else 0.5, seed=h), lone=h == 4096) for h in CONSENSUS_HYPOTHESES]
    edges += [_cedge("seed_%08x" % s, 200, params=dict(seed=s)) for s in CONSENSUS_SEED_VALUES]
    edges += [_cedge("size_%dx%d" % size, 300, size=size, params=dict(max_error=_size_error(size)), corner=size == (512, 512))
              for size in CONSENSUS_SIZES]
    edges += [_cedge("max_error_%g" % e, 300, params=dict(max_error=e)) for e in CONSENSUS_MAX_ERRORS]
    edges += [dict(name="valid2", n=None, ncols=64, nrows=64, params=dict(VALID2_PARAMS[rule_name])),
              dict(name="batch_of_every_outcome"),
              # one point twelve times: every hypothesis is degenerate, every score -1
              dict(name="one_point", n=12, ncols=64, nrows=64, params=dict(hypotheses=5, seed=1, min_inliers=lo, max_error=1.0)),
              # most hypotheses repeat a pick: identical rows, an exactly zero block at an early step of null9
              dict(name="repeated_picks", n=lo, ncols=320, nrows=240, list_seed=77,
                   params=dict(hypotheses=513, seed=3, min_inliers=lo, max_error=1.0))]
    return edges + EXTRA_CONSENSUS_EDGES[rule_name]


# entries found by the bounded searches of tests/test_check_draws_rule.py's coverage list (a pivot in the ninth column at a step the smooth
# scenes do not reach): integer_lists trials under the parameters given
EXTRA_CONSENSUS_EDGES = {"epipolar": [dict(name="integer_335", trial=335, n=None, ncols=64, nrows=64,          # a pivot tie at step 7
                                          params=dict(hypotheses=64, seed=335, min_inliers=8, max_error=1.0)),
                                     # the best hypothesis holds its largest |f_i| twice, and the refit depends on which row of M is left out
                                     dict(name="integer_1674", trial=1674, n=None, ncols=64, nrows=64,
                                          params=dict(hypotheses=64, seed=1674, min_inliers=8, max_error=0.0))],
                         # every record in a corner of a 2048 x 2048 frame: SUM qx^2 + qy^2 exceeds the count of the inliers, so the refit's first
                         # pivot is M[8][8] -- the ninth column at step 0, which no hypothesis of the homography rule takes (row 0 holds 1.0 in
                         # column 2) -- and the refit succeeds
                         "homography": [dict(name="corners", n=96, ncols=2048, nrows=2048, list_seed=5,
                                             params=dict(hypotheses=64, seed=2, min_inliers=8, max_error=0.5))]}


def _another_count(pairs, size=VALID2_SIZE):
    """the second pair loses a candidate where it holds as many as the first"""
    if len({int(candidate_mask(fin, fout, *size).sum()) for fin, fout in pairs}) < len(pairs):
        pairs[1][1]["val"][0] = -3
    return pairs


def consensus_edge_lists(rule_name, e):
    """the pairs of a fixed case: the case's own list, then the lists that share its batch -- the same scene from other seeds, with other
    numbers of candidates"""
    rule = RULES[rule_name]
    name = e["name"]
    if name == "batch_of_every_outcome":
        return consensus_every_outcome_batch(rule_name)
    if name == "valid2":
        fin, fout = valid2_lists(rule_name)
        n = len(fin)
        return dict(e, n=n), _another_count([(fin, fout), integer_lists(1, n)])
    if name == "one_point":
        x, y = np.full(e["n"], 20), np.full(e["n"], 30)
        other = integer_lists(2, e["n"])
        other[1]["val"][0] = -3
        return e, [(records(x, y, 1), records(x + 1, y - 1)), other]
    if name.startswith("integer_"):
        fin, fout = integer_lists(e["trial"])
        return dict(e, n=len(fin)), _another_count([(fin, fout), integer_lists(e["trial"] + 1, len(fin))])
    n, ncols, nrows = e["n"], e["ncols"], e["nrows"]
    if name == "corners":
        pairs = []
        for i in range(2):
            fin, fout = scene_lists(rule, 6000, ncols, nrows, e["list_seed"] + i)
            far = np.ones(len(fin), bool)
            for fl in (fin, fout):
                far &= (np.abs(fl["x"] - ncols // 2) > 0.8 * (ncols // 2)) & (np.abs(fl["y"] - nrows // 2) > 0.8 * (nrows // 2))
            assert far.sum() >= n
            fin, fout = fin[far][:n].copy(), fout[far][:n].copy()
            pairs.append(_thin(fin, fout, ncols, nrows, n - 16 * i, e["list_seed"] + i))
        return e, pairs
    if name == "repeated_picks":
        fin, fout = scene_lists(rule, n, ncols, nrows, e["list_seed"])
        short = scene_lists(rule, n, ncols, nrows, e["list_seed"] + 1)
        short[1]["val"][0] = -3                     # (one candidate too few)
        return e, [(fin, fout), short]
    kinds = (n // 2 + 3, max(1, n // 80))
    pairs = []
    for i in range(2):
        fin, fout = scene_lists(rule, n, ncols, nrows, e["list_seed"] + i, kinds)
        if e.get("corner") and i == 0:              # working coordinates of exactly -1: x = 0 and y = 0 on a frame of 2^j columns and rows
            fin["x"][1], fin["y"][2], fout["x"][3], fout["y"][4] = 0.0, 0.0, 0.0, 0.0
        cands = int(candidate_mask(fin, fout, ncols, nrows).sum())
        m = e["m"] if e["m"] is not None and i == 0 else cands - i * (40 + n // 50)
        if e.get("lone") and i == 1:
            m = rule.min_inliers - 1
        _thin(fin, fout, ncols, nrows, m, e["list_seed"] + i)
        pairs.append((fin, fout))
    return e, pairs


def draw_consensus(rule_name, seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 31 if rule_name == "epipolar" else 32])
    span = int(rng.integers(0, 4))
    n = int(rng.integers(*[(40, 400), (400, 3000), (400, 3000), (GATHER_TILE + 1, 12001)][span]))
    kind = int(rng.integers(0, 5))
    j = int(rng.integers(6, 16))
    ncols, nrows = [(int(rng.integers(64, 65536)), int(rng.integers(64, 65536))), (1 << j, int(rng.integers(64, (1 << j) + 1))),
                    ((1 << j) + 1, int(rng.integers(64, (1 << j) + 1))), (int(rng.integers(64, (1 << j) + 1)), (1 << j) + 1),
                    SCENE_SIZE][kind]
    s = (CONSENSUS_SEED_VALUES + [None, None])[int(rng.integers(0, len(CONSENSUS_SEED_VALUES) + 2))]
    scale = max(ncols / float(SCENE_SIZE[0]), nrows / float(SCENE_SIZE[1]))
    t = dict(name="draw%d" % seed, seed=seed, n=n, ncols=ncols, nrows=nrows, list_seed=int(rng.integers(0, 1 << 30)),
             kinds_start=int(rng.integers(0, max(1, n // 8))), kinds_step=int(rng.integers(1, max(2, n // 50))), npairs=int(rng.integers(2, 5)))
    t["params"] = dict(hypotheses=int(rng.choice([1, 4, 5, 64, 64, 511, 512, 513, 1001])), seed=int(rng.integers(0, 1 << 32)) if s is None else s,
                       min_inliers=int(rng.choice([RULES[rule_name].min_inliers, 8, 20])),
                       max_error=float(np.float32(float(rng.choice(CONSENSUS_MAX_ERRORS)) * scale)))
    return t


def consensus_draw_lists(rule_name, t):
    pairs = []
    for i in range(t["npairs"]):
        fin, fout = scene_lists(RULES[rule_name], t["n"], t["ncols"], t["nrows"], (t["list_seed"] + i) % (1 << 32), (t["kinds_start"] + i, t["kinds_step"]))
        cands = int(candidate_mask(fin, fout, t["ncols"], t["nrows"]).sum())
        _thin(fin, fout, t["ncols"], t["nrows"], cands - i * (1 + t["n"] // 60), t["list_seed"] + i)       # another number of candidates in every pair
        pairs.append((fin, fout))
    return pairs


# ------------------------------------------------------------------------------------------------------------ consensus expected values
@contextlib.contextmanager
def patched(mod, **names):
    """module attributes replaced for the time of the block (the restatements look their helpers up when they are called)"""
    old = {k: getattr(mod, k) for k in names}
    for k, v in names.items():
        setattr(mod, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


def cover_of(events, cover=None):
    """the branches of null9 a list of trace events went through: ("pc8", k), ("pc<8", k), ("tie", k), ("swap", k), ("fail", kind, k)"""
    cover = set() if cover is None else cover
    for ev in events:
        k = ev["k"]
        if ev["fail"]:
            cover.add(("fail", ev["fail"], k))
            continue
        cover.add(("pc8" if ev["pc8"] else "pc<8", k))
        if ev["tie"]:
            cover.add(("tie", k))
        if ev["row_swap"] or ev["col_swap"]:
            cover.add(("swap", k))
    return cover


def consensus_expected(rule_name, t, fin, fout):
    """the rule's (out, model record), the scores it decided on (None when it never scored) and null9's branches on the way"""
    rule = RULES[rule_name]
    mod = rule.mod
    seen, events = {}, []
    original = mod.scores_expected

    def spy(*a):
        seen["scores"] = original(*a)
        return seen["scores"]
    with patched(mod, scores_expected=spy, null9=functools.partial(ee.null9, trace=events)):
        out, model = getattr(mod, rule.expected)(fin, fout, t["ncols"], t["nrows"], **t["params"])
    return out, model, seen.get("scores"), cover_of(events)


def _consensus_case(rule_name, t, pairs):
    want = [consensus_expected(rule_name, t, fin, fout) for fin, fout in pairs]
    return _readonly(dict(rule=rule_name, t=t, pairs=[x for p in pairs for x in p], want_out=[w[0] for w in want], want_model=[w[1] for w in want],
                          scores=[w[2] for w in want], cover=[w[3] for w in want]))


@functools.lru_cache(maxsize=None)
def consensus_case(rule_name, seed):
    t = draw_consensus(rule_name, seed)
    return _consensus_case(rule_name, t, consensus_draw_lists(rule_name, t))


@functools.lru_cache(maxsize=None)
def consensus_edge_case(rule_name, name):
    edges = consensus_edges(rule_name)
    e = edges[[x["name"] for x in edges].index(name)]
    return _consensus_case(rule_name, *consensus_edge_lists(rule_name, e))


def _tail(flags, trip):
    """(inliers, others) among the candidates of a loop's last partial trip; None when the count is a multiple of the trip"""
    m = len(flags)
    if m % trip == 0:
        return None
    tail = flags[m - m % trip:]
    return int(tail.sum()), int((~tail).sum())


def consensus_facts(c):
    rule, t = RULES[c["rule"]], c["t"]
    facts = []
    for i in range(len(c["want_out"])):
        fin, fout, out, model, scores = c["pairs"][2 * i], c["pairs"][2 * i + 1], c["want_out"][i], c["want_model"][i], c["scores"][i]
        cand = candidate_mask(fin, fout, t["ncols"], t["nrows"])
        kept = (out["val"] == KLT_TRACKED)[cand]                    # the final pass' inliers, in candidate order
        f = dict(valid=int(model["valid"]), m=int(cand.sum()), flagged=int((~kept).sum()), kept=int(kept.sum()), best=int(model["hypothesis"]),
                 tie=False, below=False, singular=False, few=int(cand.sum()) < t["params"]["min_inliers"],
                 tails={trip: _tail(kept, trip) for trip in (SCORE_TRIP, SUM_TRIP, FINAL_TRIP)},
                 tile_candidates=[int(cand[k:k + GATHER_TILE].sum()) for k in range(0, len(fin), GATHER_TILE)])
        assert f["flagged"] == int((out["val"] == rule.outlier).sum()) - int((fout["val"] == rule.outlier).sum())
        if scores is not None:
            top = int(scores.max())
            f["tie"] = bool((scores == top).sum() >= 2 and top >= t["params"]["min_inliers"])
            f["singular"] = top < 0
            f["below"] = bool(0 <= top < t["params"]["min_inliers"])
            f["degenerate"] = int((scores < 0).sum())
        facts.append(f)
    return facts


# ------------------------------------------------------------------------------------------------------------------ consensus trial
C_IN, C_OUT, C_REC = 500, 510, 520


def run_consensus_trial(ctx, c):
    """klt_<rule>_check on every pair alone, then klt_<rule>_check_batch_async over the pairs (lists of equal length and differing candidate
    counts) against the rule: every byte of `out` and of the model record, the count of flagged records, klt_<rule>_check_path.  Returns
    None or the first difference."""
    rule, t, n = RULES[c["rule"]], c["t"], c["t"]["n"]
    name = rule.name
    npairs = len(c["want_out"])
    check, path = getattr(ctx, name + "_check"), getattr(ctx, name + "_check_path")
    getattr(ctx, "set_%s_params" % name)(ncols=t["ncols"], nrows=t["nrows"], **t["params"])
    for i in range(npairs):
        fin, fout, want_out, want_model = c["pairs"][2 * i], c["pairs"][2 * i + 1], c["want_out"][i], c["want_model"][i]
        got_out, got_model, flagged = check(fin, fout)
        bad = model_differ(got_out, got_model, want_out, want_model, "klt_%s_check, pair %d" % (name, i), rule.dtype)
        if bad:
            return bad
        want_flagged = int((want_out["val"] == rule.outlier).sum()) - int((fout["val"] == rule.outlier).sum())
        if flagged != want_flagged:
            return "pair %d: %d records flagged, %d expected" % (i, flagged, want_flagged)
        if path() != 1:
            return "klt_%s_check_path %d after a single call" % (name, path())
        ctx.featbuf_upload(C_IN + i, fin)
        ctx.featbuf_upload(C_OUT + i, fout)
    getattr(ctx, name + "_check_batch_async")([(C_IN + i, C_OUT + i, C_REC + i) for i in range(npairs)], n)
    ctx.sync()
    if path() != 2:
        return "klt_%s_check_path %d after a batch" % (name, path())
    for i in range(npairs):
        bad = model_differ(ctx.featbuf_download(C_OUT + i, n), getattr(ctx, name + "_download")(C_REC + i), c["want_out"][i], c["want_model"][i],
                           "batch of %d, pair %d" % (npairs, i), rule.dtype)
        if bad:
            return bad
        if ctx.featbuf_download(C_IN + i, n).tobytes() != c["pairs"][2 * i].tobytes():
            return "batch of %d, pair %d: the `in` list was written" % (npairs, i)
    return None


# ------------------------------------------------------------------------------------------------------------------------- crowding
def crowd_grid(ncols, nrows, min_distance):
    """fill_crowd_grid (csrc/api_crowd.hip): cells of `side` >= max(16, min_distance) pixels, doubled until there are at most 65 536"""
    side = max(min_distance, CROWD_MIN_SIDE)
    while True:
        gx, gy = (ncols + side - 1) // side, (nrows + side - 1) // side
        if gx * gy <= CROWD_MAX_CELLS:
            return side, gx, gy
        side *= 2


def scan_class(ncells):
    """how the scan of the resolve kernel's 1024 lanes meets the cells: per = ceil(ncells / 1024) cells a lane"""
    if ncells == 1:
        return "one cell"
    if ncells < CROWD_SCAN_LANES:
        return "fewer cells than lanes"
    if ncells == CROWD_SCAN_LANES:
        return "a cell a lane"
    per = (ncells + CROWD_SCAN_LANES - 1) // CROWD_SCAN_LANES
    if ncells == CROWD_MAX_CELLS:
        return "64 cells a lane, all full"
    return "2 cells a lane, lanes idle" if per == 2 else "3 cells and more a lane"


def border_cluster(ncols, nrows, r, side, pairs, seed):
    """crowd_expected.border_pairs, and `pairs` more pairs exactly r and r + 1 apart across drawn borders of the cells all over the frame
    (the last cell column and row among them), in x, in y and diagonally; ages drawn"""
    rng = np.random.default_rng([seed, 41])
    gx, gy = (ncols + side - 1) // side, (nrows + side - 1) // side
    pts = []
    for k in range(pairs):
        gap = r + k % 2
        lo = gap // 2 + 1
        bx = side * int(rng.integers(1, gx)) if gx > 1 else side
        by = side * int(rng.integers(1, gy)) if gy > 1 else side
        kind = k // 2 % 3
        if kind == 0:
            pts += [(bx - lo, by + 5), (bx - lo + gap, by + 5)]
        elif kind == 1:
            pts += [(bx + 5, by - lo), (bx + 5, by - lo + gap)]
        else:
            pts += [(bx - lo, by - lo), (bx - lo + gap, by - lo + gap)]
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    pts = pts[(pts[:, 0] >= 0) & (pts[:, 0] < ncols) & (pts[:, 1] >= 0) & (pts[:, 1] < nrows)]
    first = ce.border_pairs(ncols, nrows, r, side)[0] if ncols > 12 * side and nrows > 5 * side else ce.records([], [])
    out = np.concatenate([first, ce.records(pts[:, 0] + np.float32(0.5), pts[:, 1] + np.float32(0.25))])
    out["aux"] = np.arange(len(out))
    return out, ce.crowd_records(rng.integers(0, 3, len(out)))


def _age_extremes(prev, seed):
    """INT32_MAX, INT32_MAX - 1 and negative ages at drawn places"""
    rng = np.random.default_rng([seed, 42])
    where = rng.permutation(len(prev))[:max(3, len(prev) // 10)]
    prev["age"][where] = rng.choice([ce.INT32_MAX, ce.INT32_MAX - 1, -1, -ce.INT32_MAX - 1, -7], len(where))
    prev["age"][where[:3]] = [ce.INT32_MAX, ce.INT32_MAX - 1, -5]
    return prev


def _crowd_edge(name, size, d, n=600, make="random", **more):
    return dict(dict(name=name, ncols=size[0], nrows=size[1], d=d, n=n, make=make, list_seed=3000 + n), **more)


CROWD_CELL_FRAMES = {1: (11, 9), 1023: (33 * 16 - 5, 31 * 16 - 7), 1024: (512, 512), 1025: (41 * 16 - 5, 25 * 16), 2049: (683 * 16 - 1, 3 * 16 - 15)}
CROWD_EDGES = (
    [_crowd_edge("cells_%dx%d" % size, size, 10, 300, "border") for size in ((4096, 4096), (4097, 4096), (4096, 4097), (65535, 65535))]
    + [_crowd_edge("d17", (320, 240), 17, 300, "border"), _crowd_edge("d65536", (320, 240), 65536, 300), _crowd_edge("d_int32_max", (320, 240), 0x7fffffff, 300),
       _crowd_edge("one_cell_row", (5000, 10), 10), _crowd_edge("one_cell_column", (10, 5000), 10)]
    + [_crowd_edge("ncells_%d" % k, CROWD_CELL_FRAMES[k], 10) for k in (1, 1023, 1024, 1025, 2049)]
    + [_crowd_edge("n1_on_4k", (3840, 2160), 10, 1), _crowd_edge("n3_on_4k", (3840, 2160), 10, 3, "close")]
    + [_crowd_edge("batch_above_lds", (320, 240), 3, CROWD_LDS_STATES + 1, kinds=False),
       _crowd_edge("batch_across_lds", (320, 240), 3, CROWD_LDS_STATES + 1, kinds=False, short=True),
       _crowd_edge("chain_in_scratch", (3000, 300), 10, CROWD_LDS_STATES + 1, "chain"), _crowd_edge("age_extremes", (320, 240), 10, 600, ages=True)])
CROWD_EDGE_NAMES = [e["name"] for e in CROWD_EDGES]
CROWD_CHAIN = 200


def crowd_lists(t):
    """the (out, prev) lists of a case: two or three of equal length"""
    n, ncols, nrows, seed = t["n"], t["ncols"], t["nrows"], t["list_seed"]
    r = t["d"] - 1
    side = crowd_grid(ncols, nrows, t["d"])[0]
    lists = []
    for i in range(t.get("nlists", 2)):
        if t["make"] == "border":
            out, prev = border_cluster(ncols, nrows, r, side, n // 2, seed + i)
            out, prev = out[:n], prev[:n]
            if len(out) < n:
                more = ce.random_list(n - len(out), ncols, nrows, seed + 9 + i)
                out, prev = np.concatenate([out, more[0]]), np.concatenate([prev, more[1]])
        elif t["make"] == "close":                  # three records of which two share a pixel
            out, prev = ce.records([1900.5, 1900.25, 7.0 + i], [1000.0, 1000.5, 2100.0]), ce.crowd_records([0, 2 - i, 1])
        elif t["make"] == "chain":
            a, b = ce.chain(CROWD_CHAIN, r, x0=3.0 + i)
            c, d = ce.random_list(n - CROWD_CHAIN, ncols, nrows, seed + i)
            out, prev = np.concatenate([a, c]), np.concatenate([b, d])
        else:
            out, prev = ce.random_list(n, ncols, nrows, seed + i, max_age=t.get("max_age", 4))
            if n >= 160 and t.get("kinds", True):
                ce.non_candidate_kinds(out, ncols, nrows, start=t.get("kinds_start", 1) + i, step=t.get("kinds_step", max(1, n // 37)))
        if t.get("ages"):
            _age_extremes(prev, seed + i)
        if t.get("short") and i == 1:
            out["val"][-1] = -3                     # CROWD_LDS_STATES candidates in a list of one record more
        elif i:
            out["val"][n // 2:n // 2 + i * (n // 60)] = -3       # another number of candidates in every list
        lists.append((out, prev))
    return lists


def draw_crowd(seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 33])
    span = int(rng.integers(0, 3))
    n = int(rng.integers(*[(160, 600), (600, 4000), (4000, 9000)][span]))
    big = int(rng.integers(0, 4)) == 0
    lim = 65536 if big else 2000
    return dict(name="draw%d" % seed, seed=seed, n=n, ncols=int(rng.integers(20, lim)), nrows=int(rng.integers(20, lim)),
                d=int(rng.choice([1, 2, 3, 10, 16, 17, 33, 100])), make="random", list_seed=int(rng.integers(0, 1 << 30)), max_age=int(rng.integers(0, 6)),
                kinds_start=int(rng.integers(0, n // 8)), kinds_step=int(rng.integers(1, max(2, n // 37))), nlists=int(rng.integers(2, 4)),
                ages=bool(rng.integers(0, 2)))


def _crowd_case(t):
    lists = crowd_lists(t)
    want = [ce.crowd_check_expected(out, prev, t["ncols"], t["nrows"], t["d"]) for out, prev in lists]
    bare = [ce.crowd_check_expected(l[0], None, t["ncols"], t["nrows"], t["d"]) for l in lists[:2]]       # without a previous step
    return _readonly(dict(t=t, outs=[l[0] for l in lists], prevs=[l[1] for l in lists], want_out=[w[0] for w in want], want_crowd=[w[1] for w in want],
                          bare_out=[b[0] for b in bare], bare_crowd=[b[1] for b in bare]))


@functools.lru_cache(maxsize=None)
def crowd_case(seed):
    return _crowd_case(draw_crowd(seed))


@functools.lru_cache(maxsize=None)
def crowd_edge_case(name):
    return _crowd_case(CROWD_EDGES[CROWD_EDGE_NAMES.index(name)])


def crowd_facts(c):
    t = c["t"]
    side, gx, gy = crowd_grid(t["ncols"], t["nrows"], t["d"])
    cands = [int(ce.candidate_mask(o, t["ncols"], t["nrows"]).sum()) for o in c["outs"]]
    return dict(side=side, gx=gx, gy=gy, ncells=gx * gy, scan=scan_class(gx * gy), candidates=cands,
                kept=[int((w["val"] == 1).sum()) for w in c["want_crowd"]], crowded=[int((w["val"] == 2).sum()) for w in c["want_crowd"]],
                lds=t["n"] <= CROWD_LDS_STATES)


def crowd_differ(got_out, got_crowd, want_out, want_crowd, what):
    """None, or what differs: every byte of `out` and of the crowd records (the lists hold NaN coordinates, and -0 is not +0)"""
    for name, got, want in (("out", got_out, want_out), ("crowd", np.asarray(got_crowd).view(ce.CROWD_DTYPE), want_crowd)):
        if len(got) != len(want):
            return "%s: %d %s records for %d" % (what, len(got), name, len(want))
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1))
            return "%s: %d of %d %s records differ, first at %d: got %r, want %r" % (what, bad.size, len(got), name, bad[0], got[bad[0]], want[bad[0]])
    return None


K_OUT, K_PREV, K_REC = 540, 550, 560


def run_crowd_trial(ctx, c):
    """klt_crowd_check on every list alone with its previous step, on the first one without, then klt_crowd_check_batch_async over the
    lists (the second one without a previous step) against the rule: every byte of `out` and of the crowd records, the crowded count,
    klt_crowd_check_path, at least one round.  Returns None or the first difference."""
    t, n = c["t"], c["t"]["n"]
    nl = len(c["outs"])
    ctx.set_crowd_params(ncols=t["ncols"], nrows=t["nrows"], min_distance=t["d"])
    for i in range(nl + 1):
        k = i % nl
        prev = c["prevs"][k] if i < nl else None
        want_out, want_crowd = (c["want_out"][k], c["want_crowd"][k]) if i < nl else (c["bare_out"][0], c["bare_crowd"][0])
        got_out, got_crowd, flagged = ctx.crowd_check(c["outs"][k], prev)
        bad = crowd_differ(got_out, got_crowd, want_out, want_crowd, "klt_crowd_check, list %d%s" % (k, "" if i < nl else " without prev"))
        if bad:
            return bad
        if flagged != int((want_crowd["val"] == 2).sum()):
            return "list %d: %d records crowded, %d expected" % (k, flagged, int((want_crowd["val"] == 2).sum()))
        if ctx.crowd_check_path() != 1:
            return "klt_crowd_check_path %d after a single call" % ctx.crowd_check_path()
        if ctx.crowd_check_rounds() < 1:
            return "list %d: %d rounds" % (k, ctx.crowd_check_rounds())
    triples = []
    for i in range(nl):
        ctx.featbuf_upload(K_OUT + i, c["outs"][i])
        ctx.featbuf_upload(K_PREV + i, c["prevs"][i].view(FEAT_DTYPE))
        triples.append((K_OUT + i, K_PREV + i if i != 1 else -1, K_REC + i))
    ctx.crowd_check_batch_async(triples, n)
    ctx.sync()
    if ctx.crowd_check_path() != 2:
        return "klt_crowd_check_path %d after a batch" % ctx.crowd_check_path()
    if ctx.crowd_check_rounds() < 1:
        return "batch: %d rounds" % ctx.crowd_check_rounds()
    for i in range(nl):
        want_out, want_crowd = (c["want_out"][i], c["want_crowd"][i]) if i != 1 else (c["bare_out"][1], c["bare_crowd"][1])
        bad = crowd_differ(ctx.featbuf_download(K_OUT + i, n), ctx.crowd_download(K_REC + i, n), want_out, want_crowd, "batch of %d, list %d" % (nl, i))
        if bad:
            return bad
        if ctx.featbuf_download(K_PREV + i, n).tobytes() != c["prevs"][i].tobytes():
            return "batch of %d, list %d: the previous step's records were written" % (nl, i)
    return None


# ------------------------------------------------------------------------------------------------------------------------ the tables
EPIPOLAR_EDGES, HOMOGRAPHY_EDGES = consensus_edges("epipolar"), consensus_edges("homography")
EPIPOLAR_EDGE_NAMES, HOMOGRAPHY_EDGE_NAMES = [e["name"] for e in EPIPOLAR_EDGES], [e["name"] for e in HOMOGRAPHY_EDGES]
EPIPOLAR_SEEDS = list(range(16))
HOMOGRAPHY_SEEDS = list(range(16))
CROWD_SEEDS = list(range(12))
