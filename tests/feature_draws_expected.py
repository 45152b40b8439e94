"""Seeded random draws for gain / bias tracking, per-feature track quality and the motion-model check: the drawn parameter sets (in the
style of tests/draws_expected.py, whose vocabulary, frames and lists they reuse), their expected records from the numpy restatements of the
three rules (light_expected.light_track, quality_expected.quality_expected, model_expected.motion_check_expected -- nothing is restated
here), and the trial functions that run the HIP path against them.  The committed tables below are what tests/test_feature_draws_rule.py
(no GPU) and tests/test_gpu_feature_draws.py run; tests/fuzz/fuzz_parity.py --light / --quality / --model runs the same trial functions
on fresh seeds.  Nothing here needs a GPU until a trial function is handed a context.

What is dealt round and what is drawn: the window of a light or quality draw is LIGHT_WINDOWS[seed % 14], and a 7x7 light draw's list
form is LIGHT_FORMS_7[(seed // 14) % 8] -- the table must hold every one of them, and fresh seeds walk through them; everything else
comes from the seed's generator."""
import contextlib
import functools
import inspect

import numpy as np

import light_expected as le
import model_expected as me
import quality_expected as qe
from draws_expected import MAX_PIXELS, QUAD_FEATURES, _size, differ, tc_of_track, track_frames, track_list
from helpers import make_tc, params_from_tc
from light_expected import KLT_OOB, KLT_SMALL_DET, KLT_TRACKED, light_track
from model_expected import (KLT_MODEL_OUTLIER, MODEL_DTYPE, candidate_mask, motion_check_expected, non_candidate_kinds, records,
                            synthetic_lists)
from quality_expected import FEAT_DTYPE, QUALITY_DTYPE, quality_expected, unmeasured_kinds

LIGHT_WINDOWS = [3, 5, 7, 7, 9, 11, 13, 15, 17, 19, 21, 23, 27, 31]
# the list of a 7x7 light draw: a dense single list on either side of the four-feature kernel's threshold (n % 4 = 3, 0, 1, 2, 3), a batch
# whose pairs together stay just below / reach it, or a short drawn list
LIGHT_FORMS_7 = [2047, 2048, 2049, 2050, 2051, "below", "above", "short"]
U8_BLOCKS = ["none", "occlusion", "flat", "zero"]
F32_BLOCKS = U8_BLOCKS + ["negative", "overflow", "tiny", "bright"]

# The committed tables: every entry meets the conditions of tests/test_feature_draws_rule.py with the restatements alone.  A seed that
# fails one is replaced here, never skipped at run time.
LIGHT_SEEDS = [15, 58, 104, 117, 126, 129, 164, 184, 194, 207, 256, 260, 268, 303, 310, 339, 367, 371, 391]
QUALITY_SEEDS = [23, 25, 28, 35, 38, 50, 58, 61, 82, 84, 85, 88, 181, 272, 2996, 3038]
MODEL_SEEDS = [0, 1, 2, 5, 9, 13, 15, 17, 19, 29, 31, 32, 33, 36, 44, 46, 47]
FEATURE_API_SEEDS = [0, 1, 2, 3]                # (even: a selection grid, odd: a selection mask)


def window_class(window):
    """(MAXK, WCT) of track_window_class (track_plan.h): the kernel instantiation a window takes"""
    n = window * window
    if window in (7, 15):
        return (1, 7) if window == 7 else (4, 15)
    return (1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8 if n <= 512 else 16, 0)


WINDOW_CLASSES = {(1, 7), (4, 15), (1, 0), (2, 0), (4, 0), (8, 0), (16, 0)}


def _geometry(rng, window):
    """(levels, subsampling, width, height): the coarsest level holds a window and its border (draws_expected.draw_track's rule), so the
    frame's size follows the window"""
    while True:
        levels, ss = int(rng.integers(1, 5)), int(rng.choice([2, 4, 8]))
        coarse = ss ** (levels - 1)
        if (coarse * (window + 12)) ** 2 <= MAX_PIXELS:
            break
    lo = max(48, 3 * window)                       # (room for features that keep their window on the image)
    w, h = _size(rng, lambda w, h: w // coarse >= window + 12 and h // coarse >= window + 12 and min(w, h) >= lo)
    return levels, ss, w, h


def _block(rng, w, h, least=0):
    bw, bh = int(rng.integers(max(w // 6, least), max(w // 2, least + 1))), int(rng.integers(max(h // 6, least), max(h // 2, least + 1)))
    bw, bh = min(bw, w - 2), min(bh, h - 2)
    x0, y0 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
    return (y0, y0 + bh, x0, x0 + bw)


# ---------------------------------------------------------------------------------------------------------------- gain / bias tracking
def draw_light(seed):
    """the drawn parameters of light trial `seed` (a dict of plain values with draw_track's keys, printed with a failing trial)"""
    seed = int(seed)
    rng = np.random.default_rng([seed, 11])
    window = LIGHT_WINDOWS[seed % len(LIGHT_WINDOWS)]
    levels, ss, w, h = _geometry(rng, window)
    t = dict(seed=seed, levels=levels, ss=ss, window=window, w=w, h=h, texture=int(rng.integers(0, 1 << 30)))
    t["border"] = None if rng.random() < 0.6 else int(rng.integers(window // 2 + 1, 41))
    t["max_iter"] = int(rng.choice([3, 10, 25]))
    t["mr"] = None if rng.random() < 0.4 else float(rng.uniform(2.0, 30.0))
    t["retain"] = bool(rng.random() < 0.15)
    t["step_factor"] = float(rng.choice([1.0, 1.0, 1.0, 0.8, 2.0]))
    t["min_det"] = float(rng.choice([0.01, 0.01, 0.01, 0.5, 500.0]))
    t["min_disp"] = float(rng.choice([0.1, 0.1, 0.1, 0.03, 0.5]))
    t["shift"] = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
    t["dtype"] = str(rng.choice(["u8", "f32"]))
    t["block_kind"] = str(rng.choice(U8_BLOCKS if t["dtype"] == "u8" else F32_BLOCKS))
    t["block"] = _block(rng, w, h)
    t["gain"] = float(rng.uniform(0.4, 0.9))
    t["offset"] = float(np.floor(rng.uniform(0.0, 255.0 * (1.0 - t["gain"]))))      # 255 * gain + offset <= 255: no pixel clips
    form = LIGHT_FORMS_7[(seed // len(LIGHT_WINDOWS)) % len(LIGHT_FORMS_7)] if window == 7 else "short"
    t["form"] = form
    t["npairs"] = int(rng.integers(2, 5))
    if form == "short":
        t["n"], t["scattered"] = int(rng.integers(40, 601)), bool(rng.random() < 0.5)
    elif form in ("below", "above"):               # n * npairs: 2046 / 2046 / 2044, or 2048 / 2049 / 2048
        t["n"], t["scattered"] = -(-QUAD_FEATURES // t["npairs"]) - (form == "below"), True
    else:
        t["n"], t["scattered"] = int(form), True
    t["mindist"] = int(rng.integers(0, 25))
    t["lost_share"] = float(rng.uniform(0.05, 0.30))
    t["list_seed"] = int(rng.integers(0, 1 << 30))
    return t


def light_frames(t):
    """(frame 1, frame 2): draws_expected.track_frames's pair, frame 2 = gain * frame 2 + offset (no pixel clips; rounded for uint8), then
    the block kinds that track_frames does not know.  The float32 extremes are ordinary finite pixels: a negative block (sums that are
    not positive), a block whose squares overflow float32 (sq = inf), a block of frame 2 scaled by 2^-50 (alpha about 2^50: huge but
    finite), and a block of BOTH frames scaled by 2^40 (gxx * gyy and gxy * gxy overflow: the determinant, and with it the step, is NaN)."""
    f0, f1 = track_frames(t)
    lit = t["gain"] * f1.astype(np.float64) + t["offset"]
    y0, y1, x0, x1 = t["block"]
    kind = t["block_kind"]
    if t["dtype"] == "u8":
        f1 = np.floor(lit + 0.5).astype(np.uint8)
    else:
        f0, f1 = f0.astype(np.float32), lit.astype(np.float32)
    if kind == "flat":
        f1[y0:y1, x0:x1] = 117
    elif kind == "zero":
        f1[y0:y1, x0:x1] = 0
    elif kind == "negative":
        f1[y0:y1, x0:x1] = -f1[y0:y1, x0:x1] - np.float32(1.0)
    elif kind == "overflow":
        f1[y0:y1, x0:x1] = (f1[y0:y1, x0:x1] + np.float32(1.0)) * np.float32(2.0 ** 65)
    elif kind == "tiny":
        f1[y0:y1, x0:x1] = (f1[y0:y1, x0:x1] + np.float32(1.0)) * np.float32(2.0 ** -50)
    elif kind == "bright":
        f0[y0:y1, x0:x1] = f0[y0:y1, x0:x1] * np.float32(2.0 ** 40)
        f1[y0:y1, x0:x1] = f1[y0:y1, x0:x1] * np.float32(2.0 ** 40)
    return f0, f1


def _readonly(c):
    for a in c.values():
        for b in (a if isinstance(a, (list, tuple)) else [a]):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def light_case(seed):
    """everything a light trial needs, computed once with the restatement alone and never modified: pair i of the batch tracks list i
    from frame 1 into frame 2 (i even) or from frame 2 into frame 1 (i odd); the single call is pair 0"""
    from oracle import klt_oracle as ko
    t = draw_light(seed)
    tc = tc_of_track(t)
    p = params_from_tc(tc)
    f0, f1 = light_frames(t)
    pyr = [ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))]
    lists, want = [], []
    for i in range(t["npairs"]):
        fin = track_list(dict(t, list_seed=t["list_seed"] + i), p, f0, ko)
        lists.append(fin)
        want.append(light_track(p, pyr[i % 2], pyr[1 - i % 2], fin))
    return _readonly(dict(t=t, tc=tc, p=p, f0=f0, f1=f1, pyr=pyr, lists=lists, want=want))


@contextlib.contextmanager
def probed_light_level(counts):
    """light_expected.light_level replaced by a copy of its own source with one line more: behind the Newton step's `good = ...` a probe
    counts why a window was degenerate (a sum that is not positive, a sum or square that overflowed) and the steps that were not finite
    behind sums that passed and a determinant that was not small.  The copy is made from the source at run time: it cannot drift."""
    anchor = "            good = ok & ~(det < small) & np.isfinite(dx) & np.isfinite(dy)\n"
    src = inspect.getsource(le.light_level)
    assert src.count(anchor) == 1, "light_level's Newton step has changed: the probe no longer knows where to look"

    def probe(ok, det, small, dx, dy, sum1, sq1, S):
        sums = np.stack([sum1, sq1, le._chain(S), le._chain(S * S)])
        counts["not_positive"] = counts.get("not_positive", 0) + int((sums <= 0).any(axis=0).sum())
        counts["overflowed"] = counts.get("overflowed", 0) + int((~np.isfinite(sums)).any(axis=0).sum())
        counts["step_not_finite"] = counts.get("step_not_finite", 0) + int((ok & ~(det < small) & ~(np.isfinite(dx) & np.isfinite(dy))).sum())

    ns = dict(vars(le), _probe=probe)
    exec(compile(src.replace(anchor, anchor + "            _probe(ok, det, small, dx, dy, sum1[a], sq1[a], S)\n"), "<probed light_level>", "exec"), ns)
    original = le.light_level
    le.light_level = ns["light_level"]
    try:
        yield counts
    finally:
        le.light_level = original


def light_facts(c):
    """what the expected records of a light case exercise (tests/test_feature_draws_rule.py asserts on these)"""
    t, L = c["t"], c["t"]["levels"]
    statuses, nibble15, unvisited = set(), False, False
    for fin, rec in zip(c["lists"], c["want"]):
        live = fin["val"] >= 0
        statuses.update(int(v) for v in np.unique(rec["val"][live]))
        nib = np.stack([(rec["aux"].astype(np.uint32) >> (4 * r)) & 15 for r in range(L)], axis=1)
        nibble15 = nibble15 or bool((nib[live] == 15).any())
        unvisited = unvisited or bool((live & np.isin(rec["val"], (KLT_SMALL_DET, KLT_OOB)) & (nib != 0).any(axis=1) & (nib == 0).any(axis=1)).any())
    live = c["lists"][0]["val"] >= 0
    counts = {}
    with probed_light_level(counts):
        for i, fin in enumerate(c["lists"]):
            again = light_track(c["p"], c["pyr"][i % 2], c["pyr"][1 - i % 2], fin)
            assert again.tobytes() == c["want"][i].tobytes(), "the probed copy of light_level computes something else"
    return dict(statuses=statuses, nibble15=nibble15, unvisited=unvisited, live=int(live.sum()),
                tracked=int((live & (c["want"][0]["val"] == KLT_TRACKED)).sum()),
                lost=int((live & (c["want"][0]["val"] != KLT_TRACKED)).sum()), cls=window_class(t["window"]), **counts)


def light_path(t, variant, npairs):
    """klt_track_light_path after a launch of `npairs` pairs: 2 (four features per wavefront) exactly for 7x7 windows, a variant other
    than 0 and 2048 features or more in the launch"""
    return 2 if t["window"] == 7 and variant != 0 and t["n"] * npairs >= QUAD_FEATURES else 1


OPT_TRACK_VARIANT = 11
LIGHT_IN, LIGHT_OUT = 400, 410


def run_light_trial(ctx, c, variants=(0, 4)):
    """klt_track, a one-pair batch and a batch of the drawn 2 - 4 pairs under klt_set_light_params mode 1 against the rule's records
    (val, x, y, aux), under KLT_OPT_TRACK_VARIANT 0 / 4, klt_track_light_path after every launch.  Returns None or a description of the
    first difference; mode 0 and variant 4 are restored."""
    t, n = c["t"], c["t"]["n"]
    ctx.configure(c["tc"])
    ctx.upload(0, c["f0"])
    ctx.upload(1, c["f1"])
    ctx.build_pyramids(0)
    ctx.build_pyramids(1)
    for i, fin in enumerate(c["lists"]):
        ctx.featbuf_upload(LIGHT_IN + i, fin)
    pairs = [(i % 2, 1 - i % 2, LIGHT_IN + i, LIGHT_OUT + i) for i in range(t["npairs"])]

    def checks(variant):
        tag = "variant %d:" % variant
        got = ctx.track(0, 1, c["lists"][0])[0]
        yield None if ctx.track_light_path() == light_path(t, variant, 1) else "%s klt_track took path %d" % (tag, ctx.track_light_path())
        yield differ(got, c["want"][0], tag + " klt_track")
        for batch in (pairs[:1], pairs):
            ctx.track_batch_async(batch, n)
            ctx.sync()
            path = ctx.track_light_path()
            yield None if path == light_path(t, variant, len(batch)) else "%s a batch of %d took path %d" % (tag, len(batch), path)
            for i in range(len(batch)):
                yield differ(ctx.featbuf_download(LIGHT_OUT + i, n), c["want"][i], "%s batch of %d, pair %d" % (tag, len(batch), i))

    ctx.set_light_params(mode=1)
    try:
        for variant in variants:
            ctx.set_option(OPT_TRACK_VARIANT, variant)
            for bad in checks(variant):
                if bad:
                    return bad
    finally:
        ctx.set_option(OPT_TRACK_VARIANT, 4)
        ctx.set_light_params(mode=0)
    return None


# ------------------------------------------------------------------------------------------------------------------------ track quality
# "gained" / "negated": float32 frames, frame 2 = +-(gain * frame 1 + offset) rounded to float32, out == in -- windows that are perfectly
# correlated up to their rounding, whose quotient c / sqrt(a * b) lands on either side of +-1: the two clamps
QUALITY_KINDS = ["shifted", "lit", "identical", "inverted", "flat_first", "flat_second", "flat_both", "gained", "negated"]
N_UNMEASURED_KINDS = 82                         # records unmeasured_kinds overwrites


def draw_quality(seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 12])
    window = LIGHT_WINDOWS[seed % len(LIGHT_WINDOWS)]
    levels, ss, w, h = _geometry(rng, window)
    coarse = ss ** (levels - 1)
    for width in (w - w % 4 + int(rng.integers(0, 4)), w):           # a drawn ncols % 4, if the frame still fits
        if width * h <= MAX_PIXELS and width // coarse >= window + 12:
            w = width
            break
    t = dict(seed=seed, levels=levels, ss=ss, window=window, w=w, h=h, texture=int(rng.integers(0, 1 << 30)), border=None, max_iter=10,
             mr=None, retain=False, step_factor=1.0, min_det=0.01, min_disp=0.1, mindist=int(rng.integers(0, 15)))
    t["shift"] = (float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)))
    t["dtype"] = str(rng.choice(["u8", "f32"]))
    t["kind"] = str(rng.choice(QUALITY_KINDS))
    if t["kind"] in ("gained", "negated"):
        t["dtype"] = "f32"
    t["block_kind"] = "none"                       # (track_frames: the blocks of this draw are made by quality_frames)
    t["block"] = _block(rng, w, h, least=window + 6)
    t["gain"] = float(rng.uniform(0.4, 0.9))
    t["offset"] = float(np.floor(rng.uniform(0.0, 255.0 * (1.0 - t["gain"]))))
    t["scale"] = float(rng.uniform(0.3, 1.0))     # float32 frames: every pixel times this, so that they are no integers
    t["npairs"] = int(rng.integers(2, 5))
    t["n"], t["scattered"] = int(rng.integers(200, 321)), bool(rng.random() < 0.6)
    t["lost_share"] = float(rng.uniform(0.05, 0.30))
    t["kinds_start"] = int(rng.integers(0, t["n"] - N_UNMEASURED_KINDS))
    t["kinds_share"] = float(rng.choice([0.6, 1.0]))
    t["free_share"] = float(rng.uniform(0.1, 0.3))
    t["list_seed"] = int(rng.integers(0, 1 << 30))
    return t


def quality_frames(t):
    f0, f1 = track_frames(t)
    y0, y1, x0, x1 = t["block"]
    kind = t["kind"]
    if kind == "lit":
        f1 = np.floor(t["gain"] * f1.astype(np.float64) + t["offset"] + 0.5).astype(np.uint8)
    elif kind in ("identical", "gained", "negated"):
        f1 = f0.copy()
    elif kind == "inverted":
        f1 = (255 - f1).astype(np.uint8)
    if kind in ("flat_first", "flat_both"):
        f0[y0:y1, x0:x1] = 117
    if kind in ("flat_second", "flat_both"):
        f1[y0:y1, x0:x1] = 117
    if t["dtype"] == "f32":
        f0, f1 = ((f.astype(np.float64) * t["scale"]).astype(np.float32) for f in (f0, f1))
    if kind in ("gained", "negated"):
        f1 = ((f0.astype(np.float64) * t["gain"] + t["offset"]) * (1.0 if kind == "gained" else -1.0)).astype(np.float32)
    return f0, f1


def tracker_free(t):
    """kinds whose `out` is not a tracker's: identical, gained and negated frames with out == in, and the inverted frame 2 (out = in moved
    by the true shift)"""
    return t["kind"] in ("identical", "inverted", "gained", "negated")


def quality_lists(t, i, fin, tracked):
    """(in, out, {index: measured or not}) of pair i: `tracked` (the tracker's output on `fin`) with a drawn share of the records of
    unmeasured_kinds laid over both lists from a drawn start, and a drawn share of the other records of `out` replaced by positions
    that no tracker made -- anywhere a window fits, a third of them with integer coordinates, a sixth on the last column or row where
    a window still fits; with a flat block, every record whose `in` lies on it"""
    rng = np.random.default_rng([t["list_seed"], 20 + i])
    n, w, ncols, nrows = len(fin), t["window"], t["w"], t["h"]
    hw = w // 2
    kin, kout, kinds = unmeasured_kinds(fin, tracked, w, ncols, nrows, start=t["kinds_start"])
    keep = np.zeros(n, bool)
    keep[list(kinds)] = rng.random(len(kinds)) < t["kinds_share"]
    fin, fout = np.where(keep, kin, fin), np.where(keep, kout, tracked)
    y0, y1, x0, x1 = t["block"]
    on_block = (fin["x"] >= x0 + hw + 1) & (fin["x"] < x1 - hw - 2) & (fin["y"] >= y0 + hw + 1) & (fin["y"] < y1 - hw - 2)
    free = ~keep & (fin["val"] >= 0) & ((rng.random(n) < t["free_share"]) | (on_block & t["kind"].startswith("flat")))
    x, y = rng.uniform(hw, ncols - hw - 1, n), rng.uniform(hw, nrows - hw - 1, n)
    form = rng.integers(0, 6, n)
    x, y = np.where(form < 2, np.floor(x), x), np.where(form < 2, np.floor(y), y)
    x = np.where(form == 2, ncols - hw - 2 + np.where(rng.random(n) < 0.5, 0.0, 0.75), x)
    y = np.where(form == 3, nrows - hw - 2 + np.where(rng.random(n) < 0.5, 0.0, 0.75), y)
    if t["kind"].startswith("flat"):               # half of them onto the flat block, where a window fits wholly inside it
        inside = rng.random(n) < 0.5
        x = np.where(inside, rng.uniform(x0 + hw + 1, x1 - hw - 2, n), x)
        y = np.where(inside, rng.uniform(y0 + hw + 1, y1 - hw - 2, n), y)
    fout["x"][free], fout["y"][free], fout["val"][free] = x[free].astype(np.float32), y[free].astype(np.float32), KLT_TRACKED
    return fin, fout, {k: v for k, v in kinds.items() if keep[k]}


@functools.lru_cache(maxsize=None)
def quality_case(seed):
    """everything a quality trial needs (oracle and restatement alone, never modified): pair i measures list i between frame 1 and frame 2
    (i even) or the other way round (i odd).  `tracked` stands for the device tracker's output: the CPU oracle's, which the trial compares
    with the device's before it builds its lists from the latter."""
    from oracle import klt_oracle as ko
    t = draw_quality(seed)
    tc = tc_of_track(t)
    p = params_from_tc(tc)
    f0, f1 = quality_frames(t)
    pyr = [ko.Pyramids(p, f0.astype(np.float32)), ko.Pyramids(p, f1.astype(np.float32))]
    fins, tracked, lists, want, kinds = [], [], [], [], []
    for i in range(t["npairs"]):
        fin = track_list(dict(t, list_seed=t["list_seed"] + i), p, f0, ko)
        out = fin.copy()
        if t["kind"] in ("identical", "gained", "negated"):
            out["val"] = np.where(fin["val"] >= 0, KLT_TRACKED, fin["val"])
        elif t["kind"] == "inverted":
            sign = 1.0 if i % 2 == 0 else -1.0      # (frame 2 is frame 1 moved by +shift)
            live = fin["val"] >= 0
            out["x"][live], out["y"][live] = fin["x"][live] + np.float32(sign * t["shift"][0]), fin["y"][live] + np.float32(sign * t["shift"][1])
            out["val"] = np.where(live, KLT_TRACKED, fin["val"])
        else:
            ko.track_features(p, pyr[i % 2], pyr[1 - i % 2], out)
        a, b, k = quality_lists(t, i, fin, out)
        fins.append(fin), tracked.append(out), lists.append((a, b)), kinds.append(k)
        want.append(quality_expected(ko, pyr[i % 2], pyr[1 - i % 2], a, b, t["window"]))
    return _readonly(dict(t=t, tc=tc, p=p, f0=f0, f1=f1, pyr=pyr, fins=fins, tracked=tracked, lists=[x for ab in lists for x in ab],
                          want=want, kinds=kinds))


@contextlib.contextmanager
def probed_quality_record(counts):
    """quality_expected.quality_record replaced by a copy of its own source with one line more, which counts the rule's branches: a <= 0,
    b <= 0 (ncc = 0), e <= 0 (min_eig = 0) and the two clamps of ncc"""
    anchor = "        e = ((gxx + gyy) - np.sqrt(d * d + F64(4.0) * (gxy * gxy))) / F64(2.0)\n"
    src = inspect.getsource(qe.quality_record)
    assert src.count(anchor) == 1, "quality_record has changed: the probe no longer knows where to look"

    def probe(a, b, c, e):
        hit = dict(a_le_0=not a > 0, b_le_0=not b > 0, e_le_0=not e > 0)
        if a > 0 and b > 0:
            v = c / np.sqrt(a * b)
            hit.update(clamp_high=v > 1.0, clamp_low=v < -1.0, ncc_is_1=v == 1.0)
        for k, v in hit.items():
            counts[k] = counts.get(k, 0) + int(bool(v))

    ns = dict(vars(qe), _probe=probe)
    exec(compile(src.replace(anchor, anchor + "        _probe(a, b, c, e)\n"), "<probed quality_record>", "exec"), ns)
    original = qe.quality_record
    qe.quality_record = ns["quality_record"]
    try:
        yield counts
    finally:
        qe.quality_record = original


def quality_facts(c):
    from oracle import klt_oracle as ko
    t = c["t"]
    rest = np.ones(t["n"], bool)
    rest[list(c["kinds"][0])] = False
    counts = {}
    with probed_quality_record(counts):
        for i, want in enumerate(c["want"]):
            again = quality_expected(ko, c["pyr"][i % 2], c["pyr"][1 - i % 2], c["lists"][2 * i], c["lists"][2 * i + 1], t["window"])
            assert again.tobytes() == want.tobytes(), "the probed copy of quality_record computes something else"
    for i, kinds in enumerate(c["kinds"]):          # the overlay's own claims
        for k, is_measured in kinds.items():
            assert c["want"][i]["val"][k] == int(is_measured), (t, i, k)
    return dict(measured=int((c["want"][0]["val"][rest] == 1).sum()), unmeasured=int((c["want"][0]["val"] == 0).sum()),
                kinds={k - t["kinds_start"] for kinds in c["kinds"] for k in kinds}, cls=window_class(t["window"]), **counts)


def quality_differ(got, want, what):
    """None, or the first field whose bit patterns differ (NaN would equal NaN, -0 would differ from +0)"""
    if got.dtype != QUALITY_DTYPE or len(got) != len(want):
        return "%s: %d records of %r" % (what, len(got), got.dtype)
    for name in ("val", "residue", "ncc", "min_eig"):
        g, w = got[name].view(np.int32), want[name].view(np.int32)
        bad = np.flatnonzero(g != w)
        if bad.size:
            return "%s.%s: %d of %d differ, first at %d: got %r, want %r" % (what, name, bad.size, len(got), bad[0], got[bad[0]], want[bad[0]])
    return None


Q_IN, Q_OUT, Q_RES = 430, 440, 450


def run_quality_trial(ctx, c):
    """klt_track_quality, n = 1, and klt_track_quality_batch_async of the drawn 2 - 4 pairs -- twice on the same table, then with the
    pairs in reversed order -- against the rule's records, all four fields as bit patterns.  Returns None or the first difference."""
    t, n, np_ = c["t"], c["t"]["n"], c["t"]["npairs"]
    ctx.configure(c["tc"])
    ctx.set_light_params(mode=0)
    ctx.upload(0, c["f0"])
    ctx.upload(1, c["f1"])
    ctx.build_pyramids(0)
    ctx.build_pyramids(1)
    lists = []
    for i in range(np_):
        dev = c["tracked"][i]
        if not tracker_free(t):
            dev = ctx.track(i % 2, 1 - i % 2, c["fins"][i])[0]
            bad = differ(dev, c["tracked"][i], "the tracker's output for pair %d" % i, ("val", "x", "y"))
            if bad:
                return bad
        fin, fout, _ = quality_lists(t, i, c["fins"][i], dev)
        if any(fin[k].tobytes() != c["lists"][2 * i][k].tobytes() or fout[k].tobytes() != c["lists"][2 * i + 1][k].tobytes() for k in ("x", "y", "val")):
            return "pair %d: the lists made from the device tracker's output are not the case's" % i
        lists.append((fin, fout))
        ctx.featbuf_upload(Q_IN + i, fin)
        ctx.featbuf_upload(Q_OUT + i, fout)
    bad = quality_differ(ctx.track_quality(0, 1, *lists[0]), c["want"][0], "klt_track_quality")
    if bad:
        return bad
    for one in np.flatnonzero(c["want"][0]["val"] == 1)[:1]:           # (a fresh draw may measure nothing)
        bad = quality_differ(ctx.track_quality(0, 1, lists[0][0][one:one + 1], lists[0][1][one:one + 1]), c["want"][0][one:one + 1], "n = 1")
        if bad:
            return bad
    order = list(range(np_))
    for rep, order in enumerate((order, order, order[::-1])):
        ctx.track_quality_batch_async([(i % 2, 1 - i % 2, Q_IN + i, Q_OUT + i, Q_RES + k) for k, i in enumerate(order)], n)
        for k, i in enumerate(order):
            bad = quality_differ(ctx.quality_download(Q_RES + k, n), c["want"][i], "batch launch %d, pair %d in place %d" % (rep, i, k))
            if bad:
                return bad
    return None


# ------------------------------------------------------------------------------------------------------------------- motion-model check
MODEL_HYPOTHESES = [1, 4, 5, 511, 512, 513, 1001, 4096]
MODEL_MAX_ERRORS = [0.0, 0.01, 0.5, 1.0, 3.0]
MODEL_MIN_AREAS = [0.0, 1.0, 1e6]
MODEL_SEED_VALUES = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff, None]
GATHER_TILE = 8192                              # records model_gather_kernel takes per trip of its tile loop
MODEL_LENGTHS = [8191, 8192, 8193, 12289, 16384, 16385, 20000]
MODEL_M_EDGES = [255, 256, 257, 511, 512, 513, 2047, 2048, 2049]      # the look-ahead loops: 256 (scores), 512 (sums), 2048 (final) per trip


def draw_model(seed):
    seed = int(seed)
    rng = np.random.default_rng([seed, 13])
    span = int(rng.integers(0, 3))
    n = int(rng.integers(*[(20, 400), (400, 9000), (GATHER_TILE + 1, 20001)][span]))
    t = dict(seed=seed, n=n, ncols=int(rng.integers(64, 65536)), nrows=int(rng.integers(64, 65536)),
             displaced=float(rng.uniform(0.05, 0.45)), shift=float(rng.uniform(2.0, 20.0)), list_seed=int(rng.integers(0, 1 << 30)),
             kinds_start=int(rng.integers(0, max(1, n // 4))), kinds_step=int(rng.integers(1, max(2, n // 37))),
             npairs=int(rng.integers(2, 5)))
    s = MODEL_SEED_VALUES[int(rng.integers(0, len(MODEL_SEED_VALUES)))]
    t["params"] = dict(hypotheses=int(rng.choice(MODEL_HYPOTHESES)), seed=int(rng.integers(0, 1 << 32)) if s is None else s,
                       min_inliers=int(rng.choice([3, 8, 20])), max_error=float(rng.choice(MODEL_MAX_ERRORS)),
                       min_area=float(rng.choice(MODEL_MIN_AREAS)))
    return t


def model_lists(t, i=0):
    fin, fout, _, _, _ = synthetic_lists(t["n"], t["ncols"], t["nrows"], (t["list_seed"] + i) % (1 << 32), t["displaced"], t["shift"])
    non_candidate_kinds(fin, fout, t["ncols"], t["nrows"], start=t["kinds_start"] + i, step=t["kinds_step"])
    fout["val"][t["n"] // 2:t["n"] // 2 + i * (1 + t["n"] // 60)] = -3               # another number of candidates in every pair
    return fin, fout


def _thin(fin, fout, ncols, nrows, m, seed):
    """records of `out` marked lost, in a drawn order, until exactly m candidates are left"""
    cand = np.flatnonzero(candidate_mask(fin, fout, ncols, nrows))
    assert cand.size >= m
    drop = np.random.default_rng([seed, 14]).permutation(cand)[:cand.size - m]
    fout["val"][drop] = -3
    fout["x"][drop] = fout["y"][drop] = -1.0
    assert int(candidate_mask(fin, fout, ncols, nrows).sum()) == m
    return fin, fout


def _edge(name, n, size=(1920, 1080), lost=None, m=None, params=None, list_seed=None):
    return dict(name=name, n=n, ncols=size[0], nrows=size[1], lost=lost, m=m, list_seed=list_seed if list_seed is not None else 1000 + n,
                params=dict(dict(hypotheses=64, seed=0x9e3779b9, min_inliers=8, max_error=0.5, min_area=1.0), **(params or {})))


# The fixed cases beside the draws: list lengths around one and two tiles of the gather; tiles without a candidate; candidate counts on
# the edges of the three look-ahead loops; candidates in the second half of a tile's rounds only; frame sizes that fill the 16 bits of
# either half of the model record's size word (bit 31 set); and a batch of four pairs with every outcome.
MODEL_EDGES = (
    [_edge("n%d" % n, n, params=dict(hypotheses=1001) if n == 16385 else None) for n in MODEL_LENGTHS]
    + [_edge("first_tile_empty", GATHER_TILE + 3000, lost=(0, GATHER_TILE)),
       _edge("second_tile_empty", GATHER_TILE + 500, lost=(GATHER_TILE, GATHER_TILE + 500)),
       _edge("rounds_4_to_7", 2 * GATHER_TILE, lost=(0, GATHER_TILE // 2))]
    + [_edge("m%d" % m, m + 150 + m // 8, m=m) for m in MODEL_M_EDGES]
    + [_edge("size_65535x65535", 300, size=(65535, 65535)), _edge("size_640x40000", 300, size=(640, 40000)),
       _edge("ties_at_513", 400, params=dict(hypotheses=513, seed=0x80000000)),
       _edge("no_consensus", 300, params=dict(max_error=0.0, hypotheses=512, seed=0xffffffff)),
       dict(name="batch_of_every_outcome")])
MODEL_EDGE_NAMES = [e["name"] for e in MODEL_EDGES]


def edge_lists(e):
    fin, fout, _, _, _ = synthetic_lists(e["n"], e["ncols"], e["nrows"], e["list_seed"])
    if e["lost"] and e["lost"][0] == 0:            # the displaced records are the list's first: turn it round, so that they stay candidates
        fin, fout = fin[::-1].copy(), fout[::-1].copy()
    non_candidate_kinds(fin, fout, e["ncols"], e["nrows"], start=e["n"] // 2 + 3, step=max(1, e["n"] // 80))
    if e["lost"]:
        fout["val"][e["lost"][0]:e["lost"][1]] = -3
    if e["m"] is not None:
        _thin(fin, fout, e["ncols"], e["nrows"], e["m"], e["list_seed"])
    return fin, fout


def every_outcome_batch():
    """four pairs of 20 records under one set of parameters (min_area 0, 5 hypotheses): too few candidates; candidates without a
    consensus; a refitted model (valid 1, one record off it); collinear integer positions (an exact determinant 0: valid 2)"""
    ncols, nrows, n = 320, 240, 20
    params = dict(hypotheses=5, seed=0x80000000, min_inliers=8, max_error=1.0, min_area=0.0)   # (a seed under which no pick of the second pair repeats)
    x = np.arange(n, dtype=np.float64) * 5 + 20
    rs = np.random.RandomState(9)
    few_in, few_out, _, _, _ = synthetic_lists(n, ncols, nrows, 5)
    few_out["val"][7:] = -4
    fit_in, fit_out, _, _, _ = synthetic_lists(n, ncols, nrows, 6, displaced=0.0)
    fit_out["x"][11] += np.float32(9.0)
    pairs = [(few_in, few_out),
             (records(rs.uniform(10, 300, n), rs.uniform(10, 220, n), 1), records(rs.uniform(10, 300, n), rs.uniform(10, 220, n))),
             (fit_in, fit_out),
             (records(x + 20, x + 28, 1), records(x + 22, x + 30))]
    return dict(name="batch_of_every_outcome", n=n, ncols=ncols, nrows=nrows, params=params), pairs


def _expected_with_scores(fin, fout, ncols, nrows, params):
    """motion_check_expected, and the scores it decided on (None when the rule never scored)"""
    seen = {}
    original = me.scores_expected

    def spy(*a):
        r = original(*a)
        seen["scores"] = r[0]
        return r
    me.scores_expected = spy
    try:
        out, model = motion_check_expected(fin, fout, ncols, nrows, **params)
    finally:
        me.scores_expected = original
    return out, model, seen.get("scores")


def _model_case(t, pairs):
    want = [_expected_with_scores(fin, fout, t["ncols"], t["nrows"], t["params"]) for fin, fout in pairs]
    return _readonly(dict(t=t, pairs=[x for p in pairs for x in p], want_out=[w[0] for w in want], want_model=[w[1] for w in want],
                          scores=[w[2] for w in want]))


@functools.lru_cache(maxsize=None)
def model_case(seed):
    t = draw_model(seed)
    return _model_case(t, [model_lists(t, i) for i in range(t["npairs"])])


@functools.lru_cache(maxsize=None)
def model_edge_case(name):
    e = MODEL_EDGES[MODEL_EDGE_NAMES.index(name)]
    if name == "batch_of_every_outcome":
        return _model_case(*every_outcome_batch())
    return _model_case(e, [edge_lists(e)])


def model_facts(c):
    t = c["t"]
    facts = []
    for i in range(len(c["want_out"])):
        fin, fout, out, model, scores = c["pairs"][2 * i], c["pairs"][2 * i + 1], c["want_out"][i], c["want_model"][i], c["scores"][i]
        cand = candidate_mask(fin, fout, t["ncols"], t["nrows"])
        f = dict(valid=int(model["valid"]), m=int(cand.sum()), flagged=int(((out["val"] == KLT_MODEL_OUTLIER) & cand).sum()),
                 kept=int(((out["val"] == KLT_TRACKED) & cand).sum()), tie=False, below=False,
                 tile_candidates=[int(cand[k:k + GATHER_TILE].sum()) for k in range(0, len(fin), GATHER_TILE)])
        if scores is not None:
            top = int(scores.max())
            first = int(np.flatnonzero(scores == top)[0])
            f["tie"] = bool((scores == top).sum() >= 2 and top >= t["params"]["min_inliers"] and int(model["hypothesis"]) == first)
            f["tie_winner"] = first
            f["below"] = bool(top < t["params"]["min_inliers"] <= f["m"])
        facts.append(f)
    return facts


def model_differ(got_out, got_model, want_out, want_model, what, dtype=MODEL_DTYPE):
    """None, or what differs: every byte of the model record (`dtype`: the check's record) and of `out` (the lists hold NaN coordinates,
    and -0 is not +0)"""
    got_model, want_model = np.asarray(got_model, dtype).reshape(1), np.asarray(want_model, dtype).reshape(1)
    if got_model.tobytes() != want_model.tobytes():
        return "%s: model record differs: got %r, want %r" % (what, got_model[0], want_model[0])
    if len(got_out) != len(want_out):
        return "%s: %d records for %d" % (what, len(got_out), len(want_out))
    if got_out.tobytes() != want_out.tobytes():
        bad = np.flatnonzero((got_out.view(np.uint32).reshape(-1, 4) != want_out.view(np.uint32).reshape(-1, 4)).any(axis=1))
        return "%s: %d of %d records differ, first at %d: got %r, want %r" % (what, bad.size, len(got_out), bad[0], got_out[bad[0]],
                                                                              want_out[bad[0]])
    return None


M_IN, M_OUT, M_REC = 460, 470, 480


def run_model_trial(ctx, c):
    """klt_motion_check on every pair alone, then klt_motion_check_batch_async over the pairs (a drawn case: 2 - 4 lists of equal length
    from different list seeds) against the rule: every byte of `out` and of the model record, the count of flagged records,
    klt_motion_check_path, and klt_motion_model_affine of the host layer against the restatement's.  Returns None or the first difference."""
    from pyfeaturetrack_amd.backend import model_affine as host_affine
    t, n = c["t"], c["t"]["n"]
    npairs = len(c["want_out"])
    ctx.set_model_params(ncols=t["ncols"], nrows=t["nrows"], **t["params"])
    for i in range(npairs):
        fin, fout, want_out, want_model = c["pairs"][2 * i], c["pairs"][2 * i + 1], c["want_out"][i], c["want_model"][i]
        got_out, got_model, flagged = ctx.motion_check(fin, fout)
        bad = model_differ(got_out, got_model, want_out, want_model, "klt_motion_check, pair %d" % i)
        if bad:
            return bad
        want_flagged = int((want_out["val"] == KLT_MODEL_OUTLIER).sum()) - int((fout["val"] == KLT_MODEL_OUTLIER).sum())
        if flagged != want_flagged:
            return "pair %d: %d records flagged, %d expected" % (i, flagged, want_flagged)
        if ctx.motion_check_path() != 1:
            return "klt_motion_check_path %d after a single call" % ctx.motion_check_path()
        got, want = host_affine(got_model), me.model_affine(want_model)
        if want is None:
            if got[0] is not None or got[1] is not None:
                return "pair %d: klt_motion_model_affine gives a map for a record without a model" % i
        elif not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            return "pair %d: klt_motion_model_affine %r, the rule %r" % (i, got, want)
        ctx.featbuf_upload(M_IN + i, fin)
        ctx.featbuf_upload(M_OUT + i, fout)
    if npairs >= 2:
        ctx.motion_check_batch_async([(M_IN + i, M_OUT + i, M_REC + i) for i in range(npairs)], n)
        ctx.sync()
        if ctx.motion_check_path() != 2:
            return "klt_motion_check_path %d after a batch" % ctx.motion_check_path()
        for i in range(npairs):
            bad = model_differ(ctx.featbuf_download(M_OUT + i, n), ctx.model_download(M_REC + i), c["want_out"][i], c["want_model"][i],
                               "batch of %d, pair %d" % (npairs, i))
            if bad:
                return bad
            if ctx.featbuf_download(M_IN + i, n).tobytes() != c["pairs"][2 * i].tobytes():
                return "batch of %d, pair %d: the `in` list was written" % (npairs, i)
    return None


# --------------------------------------------------------------------------------- the three features together, through the Python API
def draw_feature_api(seed):
    from fb_expected import OCCLUSION_CASES
    seed = int(seed)
    rng = np.random.default_rng([seed, 15])
    name, width, height, window, levels, ss, block, n = OCCLUSION_CASES[0]
    t = dict(seed=seed, w=width, h=height, window=window, levels=levels, ss=ss, block=block, n=int(rng.integers(120, n + 1)),
             mindist=int(rng.integers(4, 12)), texture=int(rng.integers(0, 1 << 30)), model_seed=int(rng.choice([11, 0x80000000, 0xffffffff])),
             gains=[1.0] + [float(g) for g in rng.uniform(0.55, 0.95, 3)], selector="grid" if seed % 2 == 0 else "mask")
    t["offsets"] = [0.0] + [float(np.floor(rng.uniform(0.0, 255.0 * (1.0 - g)))) for g in t["gains"][1:]]
    t["grid"] = (int(rng.integers(24, 64)), int(rng.integers(24, 64)), int(rng.integers(2, 6)))
    t["mask_seed"] = int(rng.integers(0, 1 << 30))
    return t


def feature_api_frames(t):
    """four frames of tests/test_gpu_model.py's moving-block clip (background k * (1.3, -0.8), the block's texture k * BLOCK_MOTION),
    frame k lit by its own gain and offset (no pixel clips)"""
    from pyfeaturetrack_amd import synth
    base, other = synth.synth_base(t["w"], t["h"], t["texture"]), synth.synth_base(t["w"], t["h"], t["texture"] + 1)
    y0, y1, x0, x1 = t["block"]
    frames = []
    for k in range(4):
        f = synth.shift_frame(base, 1.3 * k, -0.8 * k)
        f[y0:y1, x0:x1] = synth.shift_frame(other, me.BLOCK_MOTION[0] * k, me.BLOCK_MOTION[1] * k)[y0:y1, x0:x1]
        frames.append(np.floor(t["gains"][k] * f.astype(np.float64) + t["offsets"][k] + 0.5).astype(np.uint8))
    return frames


def _api_records(fl):
    a = np.zeros(len(fl), FEAT_DTYPE)
    a["x"], a["y"], a["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return a


def run_feature_api_trial(seed):
    """tc.lightingCompensation = "gain_bias", tc.motionModelCheck = "affine", tc.trackQuality and a selection grid (even seeds) or mask
    (odd seeds) over four frames with KLTReplaceLostFeatures in between: every list equals light_track -> motion_check_expected chained
    on the host, tc.quality_last equals quality_expected on that list, tc.model_last the rule's model.  Returns None or the first call
    whose result differs."""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    from pyfeaturetrack_amd.backend import default_context
    from select_grid_expected import select_grid_expected
    from select_mask_expected import REPLACING_SOME, SELECTING_ALL, select_expected
    from draws_expected import mask_of
    verbose = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    try:
        t = draw_feature_api(seed)
        n, ncols, nrows, w = t["n"], t["w"], t["h"], t["window"]
        attrs = dict(mindist=t["mindist"], lightingCompensation="gain_bias", motionModelCheck="affine", model_seed=t["model_seed"], trackQuality=True)
        mask = None
        if t["selector"] == "grid":
            attrs["selectionGrid"] = t["grid"]
        else:
            mask = mask_of(dict(t, kind="rectangles", tail_zeros=0, any_value=False))
            attrs["selectionMask"] = mask
        tc = make_tc(levels=t["levels"], ss=t["ss"], window=w, **attrs)
        p = params_from_tc(tc)
        kw = dict(hypotheses=256, seed=t["model_seed"], min_inliers=8, max_error=1.0, min_area=1.0)
        frames = feature_api_frames(t)
        pyr = [ko.Pyramids(p, f.astype(np.float32)) for f in frames]

        def select(k, mode, start):
            img = frames[k].astype(np.float32)
            if t["selector"] == "grid":
                return select_grid_expected(p, img, n, t["grid"], mode, start)
            return select_expected(p, img, n, mode, start, mask)

        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
        want = select(0, SELECTING_ALL, None)
        bad = differ(_api_records(fl), want, "KLTSelectGoodFeatures", ("val", "x", "y"))
        stat = []
        for k in range(1, 4):
            if bad:
                return bad
            before = want
            tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
            fwd = light_track(p, pyr[k - 1], pyr[k], before)
            want, model = motion_check_expected(before, fwd, ncols, nrows, **kw)
            bad = differ(_api_records(fl), want, "frame %d: KLTTrackFeatures" % k, ("val", "x", "y"))
            if bad:
                return bad
            bad = quality_differ(np.ascontiguousarray(tc.quality_last), quality_expected(ko, pyr[k - 1], pyr[k], before, want, w),
                                 "frame %d: tc.quality_last" % k)
            if bad:
                return bad
            s = tc.model_last
            if (s["valid"], s["candidates"], s["inliers"], s["hypothesis"]) != (model["valid"], model["n_candidates"], model["n_inliers"], model["hypothesis"]):
                return "frame %d: tc.model_last %r, the rule %r" % (k, s, model)
            A = me.model_affine(model)
            if (A is None) != (s["A"] is None) or (A is not None and not (np.array_equal(s["A"], A[0]) and np.array_equal(s["t"], A[1]))):
                return "frame %d: tc.model_last's map %r / %r, the rule %r" % (k, s["A"], s["t"], A)
            stat.append("%d/%d" % (int((want["val"] == KLT_TRACKED).sum()), int((want["val"] == KLT_MODEL_OUTLIER).sum())))
            sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
            if (want["val"] < 0).any():
                want = select(k, REPLACING_SOME, want)
            bad = differ(_api_records(fl), want, "frame %d: KLTReplaceLostFeatures" % k, ("val", "x", "y"))
        t["_stat"] = "tracked/flagged per frame " + " ".join(stat)
        return bad
    finally:
        sgf.KLT_verbose, tf.KLT_verbose = verbose
        default_context().set_light_params(mode=0)      # the thread's shared context: whoever drives it directly next finds the plain tracker
