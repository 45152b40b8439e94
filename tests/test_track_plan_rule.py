"""The tracker launch rule without a GPU: plan_track (pyfeaturetrack_amd/csrc/track_plan.h, plain C++) is compiled with g++ into a small dump
program (tests/track_plan_dump.cpp) and asked about a sweep of launches; its answers are held against the Python restatements the GPU tests
plan their cases with -- lean_state_expected (QUAD_MIN, the model's lazy-capable rule), feature_draws_expected.light_path and window_class --
each left as it is, against the window classes as tests/COVERAGE.md lists them (row ext-4), and against the invariants of a plan.  Drift
between the host's rule and any of them fails here, not only where klt_track_light_path or klt_level0_lean disagrees on a GPU."""
import itertools
import os
import subprocess

import pytest

import lean_state_expected as L
from feature_draws_expected import WINDOW_CLASSES, light_path, window_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE, QUAD7, QUAD15 = range(3)
PLAIN, LIGHT = range(2)
WINDOWS = [3, 5, 7, 9, 15, 17, 31, 33]
# (the issue's list, and the lengths whose products with 3 and 16 pairs are 2046, 2049 and 2048)
COUNTS = [0, 1, 63, 64, 127, 128, 511, 512, 682, 683, 2047, 2048, 2049]
PAIRS = [None, 1, 3, 4, 16]                    # None: a single-pair launch
EDGE_PRODUCTS = {2044, 2046, 2047, 2048, 2049}
MAX_SAMPLES = 1024                             # window * window of the largest window the wave kernels take
# tests/COVERAGE.md, row ext-4: window -> instantiation <MAXK, WCT>
COVERAGE_CLASSES = {3: (1, 0), 5: (1, 0), 7: (1, 7), 9: (2, 0), 11: (2, 0), 13: (4, 0), 15: (4, 15), 17: (8, 0), 19: (8, 0), 21: (8, 0), 23: (16, 0),
                    27: (16, 0), 31: (16, 0)}
# LDS floats of the lazy kernels (track_kernels.hip): per feature a 14 x 16 patch, two 14 x 8 filtered planes and 16 floats of padding; the
# fused entry phase: two patches of 14 rows of 72 floats and the image values of 2 patches x 4 features x 8 x 8 set aside
LAZY_FLOATS, ENTRY_FLOATS = 14 * 16 + 2 * 14 * 8 + 16, 2 * 14 * 72 + 2 * 4 * 64
FIELDS = ("window", "n", "batched", "npairs", "fb", "guess", "light", "tree_sums", "variant", "order", "order_chunk", "grad7", "all_compact", "lazy_form")


def cdiv(a, b):
    return -(-a // b)


def npad(n):
    return (n + 3) & ~3


def request(window, n, npairs, fb=0, guess=0, light=0, tree_sums=0, variant=4, order=0, grad7=1, all_compact=0, lazy_form=0, batched=None):
    batched = (npairs is not None) if batched is None else batched
    return dict(window=window, n=n, batched=int(batched), npairs=npairs or 0, fb=fb, guess=guess, light=light, tree_sums=tree_sums,
                variant=variant, order=order, order_chunk=cdiv(n, 8), grad7=grad7, all_compact=all_compact, lazy_form=lazy_form)


def build_sweep():
    reqs = []
    for window, n, npairs in itertools.product(WINDOWS, COUNTS, PAIRS):
        for fb, guess, light, tree, variant, order, grad7, compact, form in itertools.product(*[(0, 1)] * 4, (0, 4), *[(0, 1)] * 4):
            reqs.append(request(window, n, npairs, fb, guess, light, tree, variant, order, grad7, compact, form))
    return reqs


def ask(exe, reqs):
    lines = [" ".join(str(q[f]) for f in FIELDS) for q in reqs]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    plans = [{k: (v if k == "refusal" else int(v)) for k, v in (f.split("=") for f in line.split())} for line in r.stdout.splitlines()]
    assert len(plans) == len(reqs)
    return list(zip(reqs, plans))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("track_plan") / "track_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "pyfeaturetrack_amd", "csrc"),
                    os.path.join(REPO, "tests", "track_plan_dump.cpp"), "-o", path], check=True)
    return path


@pytest.fixture(scope="module")
def answers(exe):
    return ask(exe, build_sweep())


def test_the_sweep_sits_on_the_rule_s_edges():
    products = {n * (p or 1) for n in COUNTS for p in PAIRS}
    assert EDGE_PRODUCTS <= products and L.QUAD_MIN in EDGE_PRODUCTS and L.QUAD_MIN - 1 in EDGE_PRODUCTS
    assert {3 * 682, 3 * 683, 16 * L.N_BATCH, L.N_LONG} <= products and L.N_BATCH in COUNTS
    assert max(w for w in WINDOWS if w * w <= MAX_SAMPLES) == 31 and 33 in WINDOWS
    assert {window_class(w) for w in WINDOWS + list(COVERAGE_CLASSES)} == WINDOW_CLASSES


def test_the_plan_is_what_the_restatements_say(answers):
    model = L.Model(1)
    seen = set()
    for q, p in answers:
        ny = q["npairs"] if q["batched"] else 1
        plain = not (q["fb"] or q["guess"] or q["light"])
        # lean_state_expected: the threshold, and which launches have a lazy form (the model speaks of plain launches under 7-tap filters)
        quad7 = q["variant"] != 0 and q["window"] == 7 and q["n"] * ny >= L.QUAD_MIN
        family = QUAD7 if quad7 else QUAD15 if q["variant"] != 0 and q["window"] == 15 and not q["light"] else WAVE
        model.window, model.variant, model.tree_sums = q["window"], q["variant"], bool(q["tree_sums"])
        capable = bool(plain and q["grad7"] and model.lazy_capable(q["n"], ny))
        assert (p["family"], bool(p["lazy_capable"])) == (family, capable), (q, p)
        assert (p["rule"], p["batched"], p["fb"], p["guess"]) == (LIGHT if q["light"] else PLAIN, q["batched"], q["fb"], q["guess"]), (q, p)
        # the window class: feature_draws_expected.window_class, and COVERAGE.md's list where it names the window
        assert (p["maxk"], p["wct"]) == window_class(q["window"]) and COVERAGE_CLASSES.get(q["window"], (p["maxk"], p["wct"])) == (p["maxk"], p["wct"]), (q, p)
        launch = q["n"] > 0 and ny > 0
        assert p["launch"] == launch, (q, p)
        # feature_draws_expected.light_path: what klt_track_light_path reports after a gain / bias launch
        want_path = light_path(q, q["variant"], ny) if q["light"] and launch else 0
        assert p["light_path"] == want_path and (want_path == 2) == (q["light"] and launch and family == QUAD7), (q, p)
        refused = launch and (q["window"] ** 2 > MAX_SAMPLES or (q["batched"] and q["fb"] and q["guess"]))
        assert (p["refusal"] != "-") == bool(refused), (q, p)
        if launch and q["window"] ** 2 > MAX_SAMPLES and not (q["batched"] and q["fb"] and q["guess"]):
            assert p["refusal"] == "unsupported_window_size", (q, p)
        seen.add((family, p["rule"], p["tree"], p["lazy"], p["entry"], p["fb"], p["guess"], p["batched"]))
    # every family under both rules, every form: a rule change cannot silently empty a branch
    assert {(f, r) for f, r, *_ in seen} == {(WAVE, PLAIN), (QUAD7, PLAIN), (QUAD15, PLAIN), (WAVE, LIGHT), (QUAD7, LIGHT)}
    for batched in (0, 1):
        assert {(QUAD7, PLAIN, 0, 1, 0, 0, 0, batched), (QUAD7, PLAIN, 0, 1, 1, 0, 0, batched), (QUAD7, PLAIN, 1, 0, 0, 0, 0, batched),
                (QUAD15, PLAIN, 1, 0, 0, 0, 0, batched), (QUAD7, PLAIN, 0, 0, 0, 1, 0, batched), (QUAD15, PLAIN, 1, 0, 0, 0, 1, batched)} <= seen


def test_the_invariants_of_a_plan(answers):
    for q, p in answers:
        ny = q["npairs"] if q["batched"] else 1
        fpw = 4 if p["family"] == QUAD7 else 1
        assert p["fpw"] == fpw, (q, p)
        # lazy => lazy_capable => the plain 7x7 quad kernel with the reference-order sums
        assert not p["lazy"] or p["lazy_capable"], (q, p)
        if p["lazy_capable"]:
            assert p["family"] == QUAD7 and not (p["tree"] or p["fb"] or p["guess"] or q["light"] or q["tree_sums"]) and q["grad7"] and p["launch"], (q, p)
        assert p["lazy"] == (p["lazy_capable"] and q["all_compact"]) and p["entry"] == (p["lazy"] and q["lazy_form"] != 0), (q, p)
        assert p["need_records"] == (not p["lazy"]), (q, p)
        if q["light"]:
            assert not p["uses_order"] and p["family"] != QUAD15 and not p["tree"] and not p["lazy_capable"], (q, p)
        assert p["tree"] == (q["tree_sums"] and not q["fb"] and not q["light"] and p["family"] != WAVE), (q, p)
        assert not (p["fb"] and p["tree"]), (q, p)
        assert p["uses_order"] == (q["order"] and not q["light"] and p["launch"]), (q, p)
        if not p["launch"]:
            assert (p["gx"], p["gy"], p["lds"], p["refusal"], p["light_path"]) == (0, 0, 0, "-", 0), (q, p)
            continue
        # the grid covers every feature, with not a wavefront to spare; with an order: eight chunks of whole wavefronts
        assert p["gy"] == ny, (q, p)
        if p["uses_order"]:
            assert p["gx"] == 8 * cdiv(q["order_chunk"], fpw) and 8 * q["order_chunk"] >= q["n"], (q, p)
        else:
            assert p["gx"] * fpw >= q["n"] > (p["gx"] - 1) * fpw, (q, p)
        # LDS: nothing with tree sums; the features' five product arrays; the lazy kernels' patches where they are larger
        if p["refusal"] != "-":
            continue
        products = fpw * 5 * npad(q["window"] ** 2) * 4
        want = 0 if p["tree"] else 4 * ENTRY_FLOATS if p["entry"] else 4 * max(4 * LAZY_FLOATS, products // 4) if p["lazy"] else products
        assert p["lds"] == want and p["lds"] <= 65536, (q, p)
        assert not p["entry"] or products <= 4 * 4 * LAZY_FLOATS <= p["lds"] <= 10240, (q, p)


def test_launches_outside_the_sweep(exe):
    """a batch without pairs launches nothing and has no lazy form; the window classes COVERAGE.md names beyond the sweep's windows"""
    empty = [request(7, 4096, 0, batched=True, all_compact=1), request(7, 4096, -1, batched=True)]
    for q, p in ask(exe, empty):
        assert (p["launch"], p["lazy_capable"], p["lazy"], p["need_records"], p["family"], p["gx"], p["refusal"]) == (0, 0, 0, 1, WAVE, 0, "-"), (q, p)
    for q, p in ask(exe, [request(w, 100, None, light=light) for w in COVERAGE_CLASSES for light in (0, 1)]):
        assert (p["maxk"], p["wct"]) == COVERAGE_CLASSES[q["window"]] == window_class(q["window"]), (q, p)
        assert (p["family"], p["gx"], p["lds"]) == (QUAD15 if q["window"] == 15 and not q["light"] else WAVE, 100, 20 * npad(q["window"] ** 2)), (q, p)
