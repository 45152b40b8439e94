"""Seeded random draws for the forward-backward check, the motion prior and the selection mask: the drawn parameter sets (in the style of
tests/fuzz/fuzz_parity.draw), their expected records composed from the CPU oracle alone (fb_expected, guess_expected,
select_mask_expected), and the trial functions that run the HIP path against them.  The fixed seed tables below are what
tests/test_draws_rule.py (no GPU) and tests/test_gpu_draws.py run; tests/fuzz/fuzz_parity.py --fb / --guess / --mask runs the same
trial functions on fresh seeds.  Nothing here needs a GPU until a trial function is handed a context."""
import copy
import functools
import math

import numpy as np

from fb_expected import KLT_FB_INCONSISTENT, fb_compose
from guess_expected import (FEAT_DTYPE, KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS, KLT_OOB, KLT_SMALL_DET, KLT_TRACKED, fb_guess_compose,
                            guess_compose, noisy_truth)
from helpers import make_tc, params_from_tc
from pyfeaturetrack_amd import synth
from select_mask_expected import REPLACING_SOME, SELECTING_ALL, KLT_NOT_FOUND, same_records, select_expected

WINDOWS = [3, 5, 7, 7, 9, 11, 13, 15, 15, 17, 21]
FB_MAX_ERRORS = [0.0, 0.05, 0.5, 1.0, 3.0, 1e9]
MAX_PIXELS = 90000
QUAD_FEATURES = 2048             # a 7x7 launch takes the four-features-per-wavefront kernel from this many features (all its pairs together)
MAX_BATCH_PAIRS = 24             # (the batched calls compare every pair's buffers with every other's: the copies are kept few)

# The committed tables: every entry meets the conditions of tests/test_draws_rule.py with the oracle alone.  A seed that fails one is
# replaced here, never skipped at run time.
TRACK_SEEDS = [1, 5, 8, 11, 20, 28, 55, 61, 65, 67, 68, 73, 87, 91, 96, 98, 102, 108, 110, 125, 142, 181, 385, 387]
MASK_LARGE_SEEDS = [1, 4, 9, 11]                                    # (frames above the prefilter's threshold: see draw_mask)
MASK_SEEDS = [1, 2, 3, 4, 6, 7, 11, 13, 16, 17, 19, 20, 25, 26, 30, 45]
API_SEEDS = [0, 1, 2, 3]                                # (the mask's form is seed % 4: int32, Pillow "1", bool, uint8)


def _size(rng, fits):
    while True:
        w, h = int(rng.integers(48, 361)), int(rng.integers(48, 361))
        if w * h <= MAX_PIXELS and fits(w, h):
            return w, h


# ------------------------------------------------------------------------------------------------------------------ tracking draws
def draw_track(seed):
    """the drawn parameters of tracking trial `seed` (a dict of plain values, printed with a failing trial)"""
    rng = np.random.default_rng([int(seed), 1])
    while True:
        levels, ss, window = int(rng.integers(1, 5)), int(rng.choice([2, 4, 8])), int(rng.choice(WINDOWS))
        coarse = ss ** (levels - 1)
        if (coarse * (window + 12)) ** 2 <= MAX_PIXELS:         # the coarsest level must hold a window and its border (as in fuzz_parity.draw)
            break
    w, h = _size(rng, lambda w, h: w // coarse >= window + 12 and h // coarse >= window + 12)
    t = dict(seed=int(seed), levels=levels, ss=ss, window=window, w=w, h=h, texture=int(rng.integers(0, 1 << 30)))
    t["border"] = None if rng.random() < 0.6 else int(rng.integers(window // 2 + 1, 41))
    t["max_iter"] = int(rng.choice([3, 10, 10, 25]))
    t["mr"] = None if rng.random() < 0.3 else float(rng.uniform(2.0, 30.0))
    t["retain"] = bool(rng.random() < 0.15)
    t["step_factor"] = float(rng.choice([1.0, 1.0, 1.0, 0.8, 2.0]))
    t["min_det"] = float(rng.choice([0.01, 0.01, 0.01, 0.5, 500.0]))
    t["min_disp"] = float(rng.choice([0.1, 0.1, 0.1, 0.03, 0.5]))
    t["fb_max_error"] = float(rng.choice(FB_MAX_ERRORS))
    t["far"] = bool(rng.random() < 0.4)
    if t["far"]:                                    # 10-60 px, and the moved texture still overlaps most of the frame
        length, angle = float(rng.uniform(10.0, max(10.5, min(60.0, 0.35 * min(w, h))))), float(rng.uniform(0, 2 * math.pi))
        t["shift"] = (length * math.cos(angle), length * math.sin(angle))
    else:
        t["shift"] = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
    # a block of frame 2 from another texture (an occlusion, as in fb_expected.occlusion_pair), or a flat block in both frames
    t["block_kind"] = str(rng.choice(["none", "occlusion", "occlusion", "flat"]))
    bw, bh = int(rng.integers(w // 6, w // 2)), int(rng.integers(h // 6, h // 2))
    x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
    t["block"] = (y0, y0 + bh, x0, x0 + bw)
    dense = window == 7 and rng.random() < 1.0 / 3.0
    t["scattered"] = bool(dense or rng.random() < 0.5)
    n = int(rng.integers(2049, 2300)) if dense else int(rng.integers(1, 601))
    if n % 4 == 0:
        n += 1 if dense else -1                     # never a multiple of 4: the last group of a four-feature kernel is short
    t["n"] = n
    t["mindist"] = int(rng.integers(0, 25))
    t["lost_share"] = float(rng.uniform(0.05, 0.30))
    t["noise"] = float(rng.choice([0.5, 2.0, 2.0]))
    t["npairs"] = int(rng.integers(2, 5))
    t["list_seed"] = int(rng.integers(0, 1 << 30))
    return t


def tc_of_track(t):
    tc = make_tc(levels=t["levels"], ss=t["ss"], window=t["window"], max_residue=t["mr"], mindist=t["mindist"],
                 max_iterations=t["max_iter"], retainTrackers=t["retain"], step_factor=t["step_factor"], min_determinant=t["min_det"],
                 min_displacement=t["min_disp"])
    if t["border"] is not None:
        tc.borderx = tc.bordery = t["border"]
    return tc


def track_frames(t):
    base = synth.synth_base(t["w"], t["h"], t["texture"])
    f0, f1 = synth.shift_frame(base, 0.0, 0.0), synth.shift_frame(base, *t["shift"])
    y0, y1, x0, x1 = t["block"]
    if t["block_kind"] == "occlusion":
        f1[y0:y1, x0:x1] = synth.shift_frame(synth.synth_base(t["w"], t["h"], t["texture"] + 1), 0.0, 0.0)[y0:y1, x0:x1]
    elif t["block_kind"] == "flat":
        f0[y0:y1, x0:x1] = 117
        f1[y0:y1, x0:x1] = 117
    return f0, f1


LOST_STATUSES = [-1, -2, -3, -4, -5, -6]


def track_list(t, p, f0, ko):
    """the input list: a selection with a drawn share of lost slots, or positions scattered over the whole image"""
    rng = np.random.default_rng([t["list_seed"], 2])
    n = t["n"]
    if t["scattered"]:
        fin = np.zeros(n, FEAT_DTYPE)
        fin["x"] = rng.uniform(0.0, t["w"] - 1.0, n).astype(np.float32)
        fin["y"] = rng.uniform(0.0, t["h"] - 1.0, n).astype(np.float32)
        fin["x"] = np.minimum(fin["x"], np.float32(t["w"] - 1))          # (the rounding to f32 must not leave the image)
        fin["y"] = np.minimum(fin["y"], np.float32(t["h"] - 1))
        fin["val"] = np.where(rng.random(n) < 0.7, rng.integers(1, 40000, n), 0)
    else:
        fin = ko.select_good_features(p, f0.astype(np.float32), n)
    lost = rng.random(n) < t["lost_share"]
    status = rng.choice(LOST_STATUSES, n)
    gone = lost & (rng.random(n) < 0.5)                # half of the lost slots keep a position, as after an edit of the list
    fin["val"][lost] = status[lost]
    fin["x"][gone] = -1.0
    fin["y"][gone] = -1.0
    return fin


def guess_kinds(t):
    """the kinds of tests/test_gpu_guess.mixed_guesses -- guesses that do not count, guesses off the image -- and one more: a position on
    the image at level 0 within `window` px of an edge, whose footprint leaves the image at a coarser level"""
    w, h = t["w"], t["h"]
    return [("val", -1), ("x", np.nan), ("y", np.nan), ("x", np.inf), ("y", -np.inf), ("x", 1e30), ("y", -1e30), ("x", -3.5), ("y", -0.25),
            ("x", w + 0.5), ("y", h + 2.0), ("x", w - 1.0), ("y", h - 0.5), ("x", "low"), ("x", "high"), ("y", "low"), ("y", "high")]


def track_guesses(t, fin):
    """truth plus noise, a drawn 30 % of the slots overlaid with a drawn kind of guess_kinds"""
    rng = np.random.default_rng([t["list_seed"], 3])
    g, _ = noisy_truth(fin, t["shift"], noise=t["noise"], seed=t["list_seed"] % (1 << 31))
    kinds = guess_kinds(t)
    n = len(fin)
    which = rng.integers(0, len(kinds), n)
    near = rng.uniform(0.0, float(t["window"]), n)
    for i in np.flatnonzero(rng.random(n) < 0.3):
        field, value = kinds[which[i]]
        if value == "low":
            value = near[i]
        elif value == "high":
            value = (t["w"] if field == "x" else t["h"]) - 1 - near[i]
        g[field][i] = value
    return g


def no_guesses(fin):
    """a list none of whose guesses counts, with positions that would matter if they did"""
    g = np.zeros(len(fin), FEAT_DTYPE)
    g["x"], g["y"] = fin["x"] + 20.0, fin["y"] - 20.0
    g["val"] = -1
    return g


def oracle_tracker(ko, p, pyr1, pyr2):
    pyr = {1: pyr1, 2: pyr2}

    def track(fl, a, b):
        ko.track_features(p, pyr[a], pyr[b], fl)
        return fl
    return track


def _same_xyv(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=(k != "val")) for k in ("x", "y", "val"))


@functools.lru_cache(maxsize=None)
def track_case(seed):
    """everything a tracking trial needs, computed once with the oracle alone and never modified: the draw, its frames and lists, and the
    expected records of every call -- plain (ko.track_features, with the aux words of the composition), guessed (guess_compose), fb /
    fb_back (fb_compose over the oracle) and fbg / fbg_back (fb_guess_compose)"""
    from oracle import klt_oracle as ko
    t = draw_track(seed)
    tc = tc_of_track(t)
    p = params_from_tc(tc)
    f0, f1 = track_frames(t)
    pyr1, pyr2 = ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))
    fin = track_list(t, p, f0, ko)
    guess = track_guesses(t, fin)
    # the anchor is the oracle's own tracker; the composition (which also gives the aux words) must agree with it on x, y, val
    plain = guess_compose(ko, p, pyr1, pyr2, fin, None)
    oracle = fin.copy()
    ko.track_features(p, pyr1, pyr2, oracle)
    assert _same_xyv(plain, oracle), "seed %d: guess_compose without a guess is not ko.track_features" % seed
    guessed = guess_compose(ko, p, pyr1, pyr2, fin, guess)
    fb, fwd, fb_back = fb_guess_compose(ko, p, pyr1, pyr2, fin, None, t["fb_max_error"])
    ofb, _, oback = fb_compose(oracle_tracker(ko, p, pyr1, pyr2), fin, t["fb_max_error"])
    assert _same_xyv(fb, ofb) and _same_xyv(fb_back, oback), "seed %d: the two forward-backward compositions differ" % seed
    fbg, fwdg, fbg_back = fb_guess_compose(ko, p, pyr1, pyr2, fin, guess, t["fb_max_error"])
    assert _same_xyv(fwd, plain) and _same_xyv(fwdg, guessed)
    c = dict(t=t, tc=tc, p=p, f0=f0, f1=f1, pyr1=pyr1, pyr2=pyr2, fin=fin, guess=guess, plain=plain, guessed=guessed, fb=fb,
             fb_back=fb_back, fbg=fbg, fbg_back=fbg_back)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def track_facts(c):
    """what the expected records of a tracking case exercise (tests/test_draws_rule.py asserts on these)"""
    t, fin, L = c["t"], c["fin"], c["t"]["levels"]
    live = fin["val"] >= 0
    every = [c[k] for k in ("plain", "guessed", "fb", "fb_back", "fbg", "fbg_back")]
    statuses = set()
    nibble15 = unvisited = False
    for rec in every:
        statuses.update(int(v) for v in np.unique(rec["val"][live]))
        nib = np.stack([(rec["aux"].astype(np.uint32) >> (4 * r)) & 15 for r in range(L)], axis=1)
        nibble15 = nibble15 or bool((nib[live] == 15).any())
        stopped = live & np.isin(rec["val"], (KLT_SMALL_DET, KLT_OOB)) & (nib != 0).any(axis=1) & (nib == 0).any(axis=1)
        unvisited = unvisited or bool(stopped.any())
    forward = c["guessed"] if t["far"] else c["plain"]          # the forward composition the draw is about
    differs = live & ((c["guessed"]["x"] != c["plain"]["x"]) | (c["guessed"]["y"] != c["plain"]["y"]) | (c["guessed"]["val"] != c["plain"]["val"]))
    keeps_and_rejects = False
    for fwd, out in ((c["plain"], c["fb"]), (c["guessed"], c["fbg"])):
        tracked = live & (fwd["val"] == KLT_TRACKED)
        keeps_and_rejects = keeps_and_rejects or bool((tracked & (out["val"] == KLT_TRACKED)).any()
                                                      and (tracked & (out["val"] == KLT_FB_INCONSISTENT)).any())
    return dict(statuses=statuses, nibble15=nibble15, unvisited=unvisited, live=int(live.sum()),
                tracked=int((live & (forward["val"] == KLT_TRACKED)).sum()), prior_differs=int(differs.sum()),
                keeps_and_rejects=keeps_and_rejects)


# --- the HIP path against a tracking case -------------------------------------------------------------------------------------------
OPT_TRACK_VARIANT, OPT_XCD_ORDER = 11, 13
FB_IN, FB_GUESS, FB_NONE, FB_OUT, FB_BACK, FB_PAIRS = 100, 101, 102, 103, 104, 200


def differ(got, want, what, fields=("val", "x", "y", "aux")):
    """None, or where the first field of the first record differs"""
    for name in fields:
        bad = np.flatnonzero(got[name] != want[name])
        if bad.size:
            return "%s.%s: %d of %d differ, first at %d: got %r, want %r" % (what, name, bad.size, len(got), bad[0], got[bad[0]], want[bad[0]])
    return None


def batch_pairs(t):
    """copies of the pair in a batched launch: the drawn 2-4, or for a 7x7 list as many as the four-feature kernel needs"""
    need = -(-QUAD_FEATURES // t["n"])
    return need if t["window"] == 7 and t["npairs"] < need <= MAX_BATCH_PAIRS else t["npairs"]


def run_track_trial(ctx, c, parts=("plain", "guess", "fb", "batch"), variants=(0, 4), orders=(0, 1)):
    """every call of the three features on one context against the expected records of case `c`, under KLT_OPT_TRACK_VARIANT 0 / 4 and
    (lists of 64 and more) KLT_OPT_TRACK_XCD_ORDER 0 / 1.  Returns None or a description of the first difference."""
    t, fin, guess, n = c["t"], c["fin"], c["guess"], len(c["fin"])
    ctx.configure(c["tc"])
    ctx.set_fb_params(max_error=t["fb_max_error"])
    ctx.upload(0, c["f0"])
    ctx.upload(1, c["f1"])
    ctx.build_pyramids(0)
    ctx.build_pyramids(1)
    ctx.featbuf_upload(FB_IN, fin)
    ctx.featbuf_upload(FB_GUESS, guess)
    ctx.featbuf_upload(FB_NONE, no_guesses(fin))
    npairs = batch_pairs(t)

    def get(fb):
        ctx.sync()
        return ctx.featbuf_download(fb, n)

    def checks(tag):
        if "plain" in parts:
            yield differ(ctx.track(0, 1, fin)[0], c["plain"], tag + " klt_track")
        if "guess" in parts:
            for name, fb_guess, want in (("identity", FB_IN, "plain"), ("invalid", FB_NONE, "plain"), ("drawn", FB_GUESS, "guessed")):
                ctx.track_guess_async(0, 1, FB_IN, fb_guess, FB_OUT, n)
                yield differ(get(FB_OUT), c[want], "%s klt_track_guess (%s guesses)" % (tag, name))
        if "fb" in parts:
            for back in (FB_BACK, -1):
                ctx.track_fb_async(0, 1, FB_IN, FB_OUT, n, back)
                yield differ(get(FB_OUT), c["fb"], "%s klt_track_fb out (back %d)" % (tag, back))
                if back >= 0:
                    yield differ(get(back), c["fb_back"], tag + " klt_track_fb back")
                ctx.track_fb_guess_async(0, 1, FB_IN, FB_GUESS, FB_OUT, n, back)
                yield differ(get(FB_OUT), c["fbg"], "%s klt_track_fb_guess out (back %d)" % (tag, back))
                if back >= 0:
                    yield differ(get(back), c["fbg_back"], tag + " klt_track_fb_guess back")
            ctx.track_fb_guess_async(0, 1, FB_IN, FB_IN, FB_OUT, n, FB_BACK)
            yield differ(get(FB_OUT), c["fb"], tag + " klt_track_fb_guess out (identity guesses)")
            yield differ(get(FB_BACK), c["fb_back"], tag + " klt_track_fb_guess back (identity guesses)")
        if "batch" in parts and "guess" in parts:               # the last pair without a guess list
            ctx.track_guess_batch_async([(0, 1, FB_IN, FB_GUESS if i < npairs - 1 else -1, FB_PAIRS + i) for i in range(npairs)], n)
            for i in range(npairs):
                yield differ(get(FB_PAIRS + i), c["guessed" if i < npairs - 1 else "plain"], "%s guess batch, pair %d of %d" % (tag, i, npairs))
        if "batch" in parts and "fb" in parts:
            ctx.track_fb_batch_async([(0, 1, FB_IN, FB_PAIRS + i, FB_PAIRS + npairs + i) for i in range(npairs)], n)
            for i in range(npairs):
                yield differ(get(FB_PAIRS + i), c["fb"], "%s fb batch out, pair %d of %d" % (tag, i, npairs))
                yield differ(get(FB_PAIRS + npairs + i), c["fb_back"], "%s fb batch back, pair %d of %d" % (tag, i, npairs))

    try:
        for variant in variants:
            for order in (orders if n >= 64 else (1,)):
                ctx.set_option(OPT_TRACK_VARIANT, variant)
                ctx.set_option(OPT_XCD_ORDER, order)
                for bad in checks("variant %d, order %d:" % (variant, order)):
                    if bad:
                        return bad
    finally:
        ctx.set_option(OPT_TRACK_VARIANT, 4)
        ctx.set_option(OPT_XCD_ORDER, 1)
    return None


# --------------------------------------------------------------------------------------------------------------------- mask draws
MASK_KINDS = ["rectangles", "bernoulli", "sparse", "lines", "tail", "window"]


PREFILTER_CANDIDATES = 262144   # a selection with more candidates than this cuts them first (mask_hist_kernel), and a replacement takes prepared scores


def draw_mask(seed, large=False):
    """`large`: a frame with more than PREFILTER_CANDIDATES candidates -- the only sizes at which the candidate prefilter and the prepared
    scores are used at all (nSkippedPixels 0 or 1, so that the frame stays near a megapixel)"""
    rng = np.random.default_rng([int(seed), 4])
    t = dict(seed=int(seed), large=bool(large), window=int(rng.choice([3, 5, 7, 9, 11, 13, 15])))
    t["border"] = None if rng.random() < 0.6 else int(rng.integers(t["window"] // 2 + 1, 41))
    tc = make_tc(window=t["window"])
    margin = int(max(t["border"] if t["border"] is not None else tc.borderx, t["window"] / 2.0))
    skip = int(rng.integers(0, 2)) if large else None
    if large:
        while True:
            t["w"], t["h"] = int(rng.integers(600, 1400)), int(rng.integers(500, 1000))
            cells = ((t["w"] - 2 * margin + skip) // (skip + 1)) * ((t["h"] - 2 * margin + skip) // (skip + 1))
            if PREFILTER_CANDIDATES * 1.05 < cells < PREFILTER_CANDIDATES * 1.4:
                break
    else:
        t["w"], t["h"] = _size(rng, lambda w, h: w - 2 * margin >= 24 and h - 2 * margin >= 24)     # a candidate grid worth masking
    t.update(skip=skip if large else int(rng.integers(0, 4)), mindist=int(rng.integers(0, 26)), smooth=bool(rng.integers(0, 2)),
             min_eig=int(rng.choice([1, 10, 200])), n=int(rng.integers(1, 601)), texture=int(rng.integers(0, 1 << 30)),
             mode=int(rng.choice([SELECTING_ALL, REPLACING_SOME])), lost_share=float(rng.choice([0.02, 0.2, 0.5, 0.9])),
             kind=str(rng.choice(MASK_KINDS)), tail_zeros=int(rng.integers(1, 16)) if rng.random() < 0.4 else 0,
             any_value=bool(rng.integers(0, 2)), mask_seed=int(rng.integers(0, 1 << 30)))
    return t


def tc_of_mask(t):
    tc = make_tc(window=t["window"], mindist=t["mindist"], nSkippedPixels=t["skip"], smoothBeforeSelecting=t["smooth"],
                 min_eigenvalue=t["min_eig"])
    if t["border"] is not None:
        tc.borderx = tc.bordery = t["border"]
    return tc


def mask_of(t):
    """the drawn mask: uint8 [h][w], 0 = never a candidate"""
    rng = np.random.default_rng([t["mask_seed"], 5])
    w, h, kind = t["w"], t["h"], t["kind"]
    m = np.ones((h, w), np.uint8)
    if kind == "rectangles":                       # zeros at arbitrary byte offsets: runs that start and end anywhere in a 16-byte piece
        for _ in range(int(rng.integers(1, 7))):
            rw, rh = int(rng.integers(1, w // 2)), int(rng.integers(1, h // 2))
            x0, y0 = int(rng.integers(0, w - rw)), int(rng.integers(0, h - rh))
            m[y0:y0 + rh, x0:x0 + rw] = 0
    elif kind == "bernoulli":                      # almost every piece mixed
        m[rng.random((h, w)) < 0.5] = 0
    elif kind == "sparse":
        m[rng.random((h, w)) < 0.01] = 0
    elif kind == "lines":
        for _ in range(int(rng.integers(1, 9))):
            m[int(rng.integers(0, h)), :] = 0
            m[:, int(rng.integers(0, w))] = 0
    elif kind == "window":                         # nothing allowed but a small window: the candidates run out
        m[:] = 0
        sw, sh = int(rng.integers(12, max(13, w // 3))), int(rng.integers(12, max(13, h // 3)))
        x0, y0 = int(rng.integers(0, w - sw)), int(rng.integers(0, h - sh))
        m[y0:y0 + sh, x0:x0 + sw] = 1
    tail = t["tail_zeros"] or (int(rng.integers(1, 16)) if kind == "tail" else 0)
    if tail:                                       # the last bytes of the plane, whatever else the mask holds
        m.reshape(-1)[-tail:] = 0
    if t["any_value"]:                             # "allowed" is any non-zero byte
        m = np.where(m != 0, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    return m


@functools.lru_cache(maxsize=None)
def mask_case(seed, large=False):
    """a mask trial's inputs and expected lists (oracle alone, never modified): `start` the list a replacement starts from (the unmasked
    selection with a drawn share lost; None for SELECTING_ALL), `want` the selection under the mask, `unmasked` without it"""
    t = draw_mask(seed, large)
    tc = tc_of_mask(t)
    p = params_from_tc(tc)
    f = synth.shift_frame(synth.synth_base(t["w"], t["h"], t["texture"]), 0.0, 0.0)
    img = f.astype(np.float32)
    mask = mask_of(t)
    start = None
    if t["mode"] == REPLACING_SOME:
        start = select_expected(p, img, t["n"])
        lost = np.random.default_rng([t["mask_seed"], 6]).random(t["n"]) < t["lost_share"]
        start["x"][lost] = -1.0
        start["y"][lost] = -1.0
        start["val"][lost] = KLT_NOT_FOUND
    want = select_expected(p, img, t["n"], t["mode"], start, mask)
    unmasked = select_expected(p, img, t["n"], t["mode"], start, None)
    # a selection on the slot's pyramid (and on scores prepared from it) reads the SMOOTHED level-0 planes whatever the draw says
    want_pyr, unmasked_pyr = want, unmasked
    if not t["smooth"]:
        q = copy.copy(p)
        q.smoothBeforeSelecting = 1
        want_pyr = select_expected(q, img, t["n"], t["mode"], start, mask)
        unmasked_pyr = select_expected(q, img, t["n"], t["mode"], start, None)
    c = dict(t=t, tc=tc, p=p, frame=f, mask=mask, start=start, want=want, unmasked=unmasked, want_pyr=want_pyr, unmasked_pyr=unmasked_pyr)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def mask_facts(c):
    t, mask, want, start = c["t"], c["mask"], c["want"], c["start"]
    n = t["w"] * t["h"]
    placed = want["val"] >= 0 if start is None else (start["val"] < 0) & (want["val"] >= 0)
    on_zero = bool((mask[want["y"][placed].astype(int), want["x"][placed].astype(int)] == 0).any())
    tail_zero = bool(n % 16 and (mask.reshape(-1)[n - n % 16:] == 0).any())
    live_overlap = False
    if start is not None and c["p"].mindist > 0:
        d = int(c["p"].mindist) - 1                # the square the walk blocks around a live feature (selectGoodFeatures.py:61)
        for f in start[start["val"] >= 0]:
            x, y = int(f["x"]), int(f["y"])
            sq = mask[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1]
            if (sq == 0).any() and (sq != 0).any():
                live_overlap = True
                break
    return dict(differs=not same_records(want, c["unmasked"]), on_zero=on_zero, tail_zero=tail_zero, live_overlap=live_overlap,
                placed=int(placed.sum()), n16=n % 16)


KLT_OPT_TOPK_PREFILTER, KLT_OPT_SELECT_PARALLEL_NMS = 5, 8
FB_SELECT = 110


def run_mask_trial(ctx, c):
    """klt_set_select_mask as a compact host mask, with a padded stride and as a device mask; under each the selection on unprepared and
    on prepared scores against the expected list; once without the candidate prefilter and once with the serial walk; then the mask is
    cleared and the unmasked selection must be back.  Returns None or a description of the first difference."""
    t, mask, start, n = c["t"], c["mask"], c["start"], c["t"]["n"]
    w, h = t["w"], t["h"]
    ctx.set_select_mask(None)
    ctx.configure(c["tc"])
    ctx.upload(0, c["frame"])
    ctx.build_pyramids(0, sync=True)
    empty = np.zeros(n, FEAT_DTYPE)
    empty["x"], empty["y"], empty["val"] = -1.0, -1.0, KLT_NOT_FOUND

    def selections(tag, masked):
        want, want_pyr = (c["want"], c["want_pyr"]) if masked else (c["unmasked"], c["unmasked_pyr"])
        got = ctx.select(0, n, t["mode"], start, False)[0]
        yield None if same_records(got, want) else "%s: selection" % tag
        got = ctx.select(0, n, t["mode"], start, True)[0]
        yield None if same_records(got, want_pyr) else "%s: selection on the pyramid's planes" % tag
        ctx.select_prepare(0)
        ctx.featbuf_upload(FB_SELECT, empty if start is None else np.array(start, FEAT_DTYPE))
        ctx.select_begin(0, t["mode"], True, FB_SELECT, n)
        ctx.select_finish()
        got = ctx.featbuf_download(FB_SELECT, n)
        yield None if same_records(got, want_pyr) else "%s: selection on prepared scores" % tag

    def all_forms():
        ctx.set_select_mask(np.ascontiguousarray(mask))
        yield from selections("compact host mask", True)
        wide = np.zeros((h, w + 13), np.uint8)      # what lies behind a row's end must not matter: zeros would mask
        wide[:, :w] = mask
        ctx.set_select_mask(wide[:, :w])
        yield from selections("host mask with pitch w + 13", True)
        for opt in (KLT_OPT_TOPK_PREFILTER, KLT_OPT_SELECT_PARALLEL_NMS):
            ctx.set_option(opt, 0)
            try:
                yield from selections("option %d off" % opt, True)
            finally:
                ctx.set_option(opt, 1)
        ctx.set_select_mask(None)
        dev = ctx.device_alloc(w * h)               # exactly the mask: nothing behind byte w * h - 1 is the caller's
        try:
            ctx.device_write(dev, np.ascontiguousarray(mask))
            ctx.set_select_mask_device(dev, w, h)
            yield from selections("device mask", True)
            ctx.set_select_mask_device(None, 0, 0)
        finally:
            ctx.sync()
            ctx.device_free(dev)
        yield from selections("mask cleared", False)

    try:
        for bad in all_forms():
            if bad:
                return bad
    finally:
        ctx.set_select_mask(None)
    return None


# ----------------------------------------------------------------------------------- the three features together, through the Python API
MASK_FORMS = ["int32", "pillow-1", "bool", "uint8"]


def draw_api(seed):
    rng = np.random.default_rng([int(seed), 7])
    levels, ss = [(2, 4), (2, 2), (3, 2), (1, 2)][int(rng.integers(0, 4))]
    t = dict(seed=int(seed), levels=levels, ss=ss, window=int(rng.choice([5, 7, 9, 15])), form=MASK_FORMS[int(seed) % len(MASK_FORMS)])
    tc = make_tc(levels=levels, ss=ss, window=t["window"])
    t["w"], t["h"] = _size(rng, lambda w, h: w - 2 * tc.borderx >= 60 and h - 2 * tc.bordery >= 60)
    t.update(n=int(rng.integers(40, 301)), mindist=int(rng.integers(3, 16)), fb_max_error=float(rng.choice([0.5, 1.0, 3.0])),
             texture=int(rng.integers(0, 1 << 30)), kind=str(rng.choice(["rectangles", "lines", "sparse", "bernoulli"])), tail_zeros=0,
             any_value=False, mask_seed=int(rng.integers(0, 1 << 30)),
             acceleration=(float(rng.uniform(1.5, 4.0)) * float(rng.choice([-1, 1])), float(rng.uniform(0.5, 2.0)) * float(rng.choice([-1, 1]))))
    return t


def api_mask_value(t, mask):
    """the mask as the drawn kind of object tc.selectionMask accepts"""
    if t["form"] == "int32":                       # 256 and -1 are "allowed" too: any non-zero element, not its low byte
        alt = (np.indices(mask.shape).sum(axis=0) % 2).astype(bool)
        return np.where(mask != 0, np.where(alt, 256, -1), 0).astype(np.int32)
    if t["form"] == "pillow-1":
        from PIL import Image
        return Image.fromarray((mask != 0).astype(np.uint8) * 255).convert("1")
    return (mask != 0) if t["form"] == "bool" else mask


def _api_records(fl):
    a = np.zeros(len(fl), FEAT_DTYPE)
    a["x"], a["y"], a["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return a


def run_api_trial(seed):
    """tc.selectionMask + tc.forwardBackwardCheck + KLTTrackFeatures(guess=KLTPredictConstantVelocity(...)) over four frames of an
    accelerating pan with KLTReplaceLostFeatures between the frames, against the per-call oracle compositions chained on the host.
    Returns None or the first call whose list differs."""
    from oracle import klt_oracle as ko
    from guess_expected import predict_cv
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    verbose = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    try:
        t = draw_api(seed)
        mask = mask_of(t)
        tc = make_tc(levels=t["levels"], ss=t["ss"], window=t["window"], mindist=t["mindist"], forwardBackwardCheck=True,
                     fb_max_error=t["fb_max_error"], selectionMask=api_mask_value(t, mask))
        p = params_from_tc(tc)
        base = synth.synth_base(t["w"], t["h"], t["texture"])
        ax, ay = t["acceleration"]
        frames = [synth.shift_frame(base, ax * k * (k + 1) / 2, ay * k * (k + 1) / 2) for k in range(4)]
        pyr = [ko.Pyramids(p, f.astype(np.float32)) for f in frames]
        n = t["n"]
        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
        want = select_expected(p, frames[0].astype(np.float32), n, mask=mask)
        bad = differ(_api_records(fl), want, "KLTSelectGoodFeatures", ("val", "x", "y"))
        before = want_before = None
        stat = []
        for k in range(1, 4):
            if bad:
                return bad
            guess = tf.KLTPredictConstantVelocity(before, fl) if k >= 2 else None
            g = predict_cv(want_before, want) if k >= 2 else None
            before, want_before = _api_records(fl), want
            tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl, guess=guess)
            want = fb_guess_compose(ko, p, pyr[k - 1], pyr[k], want, g, t["fb_max_error"])[0]
            bad = differ(_api_records(fl), want, "frame %d: KLTTrackFeatures" % k, ("val", "x", "y"))
            if bad:
                return bad
            stat.append("%d/%d" % (int((want["val"] == KLT_TRACKED).sum()), int((want["val"] == KLT_FB_INCONSISTENT).sum())))
            sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
            if (want["val"] < 0).any():
                want = select_expected(p, frames[k].astype(np.float32), n, REPLACING_SOME, want, mask)
            bad = differ(_api_records(fl), want, "frame %d: KLTReplaceLostFeatures" % k, ("val", "x", "y"))
        t["_stat"] = "tracked/rejected per frame " + " ".join(stat)
        return bad
    finally:
        sgf.KLT_verbose, tf.KLT_verbose = verbose
