"""The level-0 pyramid kernels at the edges of their strips, bands, segments and tiles: a restatement of the host's choice of kernel
(expected_path -- it only PLANS cases; the GPU tests assert it against klt_level0_path, so that drift fails instead of losing coverage),
the edge classes of a frame's width and height, the case tables, distinct test frames, a random draw that picks the kernel first and the
frame to reach it, and the trial function that builds a case on the HIP path and compares every plane with the CPU oracle bit for bit.
tests/test_pyramid_rule.py (no GPU) asserts what the tables cover; tests/test_gpu_l0_edges.py and tests/test_gpu_draws.py run them;
tests/fuzz/fuzz_parity.py --pyramid runs the same trial function on fresh draws.  Nothing here needs a GPU until run_pyramid_trial is
handed a context.

The launch thresholds count pixels and workgroups per LAUNCH, and a launch takes up to 32 frames: a batch of 32 small frames reaches the
kernels that single frames reach only at 1080p and beyond -- with every remainder of the width and the height, and at a fraction of the
oracle's time."""
import collections
import functools

import numpy as np

from helpers import make_tc, params_from_tc

# klt_level0_path codes (include/klt_gpu.h)
TWO_PASS, TILED_LDS, RB16, RB32, RB32_HRED, STREAM, STREAM_NO_CENTRE = range(7)
PATH_NAMES = ["two-pass", "smooth_grad_kernel", "rb 16-row", "rb 32-row", "rb 32-row + reduction", "stream", "stream, centre tap elided"]
OPT_FUSED_KERNELS, OPT_FUSED_HREDUCE, OPT_L0_STREAM = 1, 12, 21
MAX_BATCH = 32                  # KLT_MAX_BATCH: frames per launch; a longer list of equal frames is split into groups
STRIP, SEG, BAND, TILE_ROWS = 64, 160, 32, 32   # strip / tile width, the streaming kernel's segment and band, the tall tile
COL_HALO = 16                   # columns of raw frame a strip reads beyond each side
TALL_PIXELS = 1000000           # launches of at least this many pixels take the 32-row tile
STREAM_WORKGROUPS = 2048        # the streaming kernel's grid bound


@functools.lru_cache(maxsize=None)
def _tap_counts(ss, sigma):
    """(smoothing, pyramid, gradient) tap counts of the host's own tap generator at the default 7x7 window"""
    from pyfeaturetrack_amd.params import taps_from_params
    return tuple(len(g) for g, _ in taps_from_params(params_from_tc(make_tc(levels=2, ss=ss, smooth_sigma_fact=sigma))))


def expected_path(ncols, nrows, batch, f32, levels, ss, smooth_sigma_fact, stream_opt=1, hreduce_opt=1, fused_opt=1):
    """(KLT_L0_* code, merged) that klt_level0_path reports after a build of `batch` equal frames: the kernel of level 0 of the LAST group
    of at most 32 frames, and whether the gradients of that group's levels >= 1 are one launch.  Restates plan_level0
    (l0_plan.h; tests/test_l0_plan_rule.py holds the two together) and build_pyramids_batch (api_frames.hip) at the default window and
    gradient sigma."""
    group = (batch - 1) % MAX_BATCH + 1
    ns, nreduce, ngrad = _tap_counts(ss, smooth_sigma_fact)
    assert ngrad == 7
    if not fused_opt:
        return TWO_PASS, False
    merged = levels > 1 and group * (levels - 1) <= MAX_BATCH and ncols // ss <= 32767 and nrows // ss <= 32767
    if ns not in (5, 9):
        return TILED_LDS, merged
    tall = ncols * nrows * group >= TALL_PIXELS
    hred = bool(hreduce_opt) and levels > 1 and tall and ss == 4 and nreduce == 21 and nrows >= 64 and ncols >= 64
    if hred:
        grid = -(-ncols // STRIP) * -(-nrows // SEG) * group
        if stream_opt and ncols >= 2 * STRIP and grid >= STREAM_WORKGROUPS:
            return (STREAM if f32 else STREAM_NO_CENTRE), merged
        return RB32_HRED, merged
    return (RB32 if tall else RB16), merged


# ------------------------------------------------------------------------------------------------------------------------ edge classes
def col_class(ncols):
    """the last 64-column strip (or tile column) of a frame: ncols % 4 (only multiples of 4 take the aligned quad loads of the raw
    frame; the others send EVERY block down the element-by-element reflect path) and the last strip's width against the 16-column halo
    (narrower: the right halo of the full strip before it reflects at the frame's edge)"""
    r = ncols % STRIP
    width = "full" if r == 0 else "below-halo" if r < COL_HALO else "halo" if r == COL_HALO else "above-halo"
    return "mod4=%d/%s" % (ncols % 4, width)


COL_CLASSES = ["mod4=0/full", "mod4=0/below-halo", "mod4=0/halo", "mod4=0/above-halo", "mod4=1/below-halo", "mod4=1/above-halo",
               "mod4=2/below-halo", "mod4=2/above-halo", "mod4=3/below-halo", "mod4=3/above-halo"]


def row_class(nrows, seg=SEG):
    """the last segment (seg 160: the streaming kernel) or the last tile row (seg 32: the tiled kernels) of a frame.  single: the whole
    frame is one segment, top and bottom reflection in one workgroup; whole: no remainder; halo: a remainder of 1-7 rows, inside the
    vertical halo of rs + 3 rows (5 rows with 5 smoothing taps, 7 with 9), where the prologue band and the bottom reflection meet;
    last-row: one row short of a segment; band-1 / band / band+1: a remainder of 32 k - 1, 32 k, 32 k + 1 rows -- either side of a band
    boundary (the `full` flag of the last band and the condition of the u8 prefetch); part: anything else"""
    q = nrows % seg
    if nrows <= seg:
        return "single"
    if q == 0:
        return "whole"
    if q <= 7:
        return "halo"
    if q == seg - 1:
        return "last-row"
    if seg > BAND and q % BAND in (BAND - 1, 0, 1):
        return {BAND - 1: "band-1", 0: "band", 1: "band+1"}[q % BAND]
    return "part"


STREAM_ROW_CLASSES = ["single", "whole", "halo", "last-row", "band-1", "band", "band+1", "part"]
TILED_ROW_CLASSES = ["whole", "halo", "last-row", "part"]

# the remainders a draw picks from (the class lists above, as numbers)
COL_REMAINDERS = [0, 4, 8, 12, 16, 20, 60, 1, 5, 3, 15, 17, 63, 2, 6, 14, 18, 62]
STREAM_ROW_REMAINDERS = [0, 1, 2, 3, 4, 5, 7, 8, 31, 32, 33, 35, 64, 96, 128, 159]
TILED_ROW_REMAINDERS = [0, 1, 3, 7, 8, 31]


# -------------------------------------------------------------------------------------------------------------------------- case tables
# batch: frames of the build; kinds: None = every frame of the test's dtype, "mixed" = u8 and f32 frames interleaved (two groups)
Case = collections.namedtuple("Case", "table ncols nrows sigma batch levels ss fused kinds", defaults=(32, 3, 4, 1, None))


def case_id(c):
    extra = "" if (c.levels, c.ss, c.fused, c.kinds) == (3, 4, 1, None) else "-L%d-ss%d%s%s" % (
        c.levels, c.ss, "" if c.fused else "-twopass", "-" + c.kinds if c.kinds else "")
    return "%dx%dx%d-s%.2g%s" % (c.ncols, c.nrows, c.batch, c.sigma, extra)


def _narrow_rows(ncols, q):
    """the fewest segments of 160 rows (+ q) at which 32 frames of `ncols` columns fill the streaming kernel's grid bound"""
    strips = -(-ncols // STRIP)
    segs = -(-STREAM_WORKGROUPS // (strips * MAX_BATCH))
    return SEG * segs if q == 0 else SEG * (segs - 1) + q


# two or three strips wide, 21 - 32 segments high: column classes and row remainders swept together, paired one to one
_NARROW = [(128, 0, 0.1), (132, 1, 0.2), (136, 2, 0.1), (140, 3, 0.2), (144, 4, 0.1), (148, 5, 0.2), (188, 7, 0.1), (131, 8, 0.2),
           (143, 31, 0.1), (145, 32, 0.2), (191, 33, 0.1), (130, 35, 0.1), (134, 64, 0.1), (142, 96, 0.2), (146, 128, 0.1), (190, 159, 0.2),
           # (beyond the list of the issue: the classes above that it leaves with one tap count or without a case)
           # band-1 and last-row with the other tap count; a remainder equal to the vertical halo (5 rows with 5 taps, 7 with 9)
           (133, 31, 0.2), (192, 159, 0.1), (189, 5, 0.1), (187, 7, 0.2)]
STREAM_NARROW = [Case("STREAM_NARROW", nc, _narrow_rows(nc, q), s) for nc, q, s in _NARROW]
# one segment (>= 64 strips) and two segments (>= 32 strips)
STREAM_WIDE = [Case("STREAM_WIDE", nc, nr, s) for nc, nr, s in [
    (4096, 64, 0.2), (4100, 65, 0.1), (4104, 67, 0.2), (4099, 96, 0.1), (4096, 97, 0.2), (4100, 159, 0.1), (4104, 160, 0.2),
    (2048, 161, 0.1), (2049, 163, 0.2), (2052, 167, 0.1), (2066, 192, 0.2), (2110, 193, 0.2), (2048, 320, 0.2)]]
STREAM_CASES = STREAM_NARROW + STREAM_WIDE

# the smallest frames of the fused-reduction tile: >= 31 250 pixels (1 000 000 per launch of 32), sides >= 64
TILED_HRED_SMALL = [Case("TILED_HRED_SMALL", nc, nr, s) for nc, nr, s in [
    (489, 64, 0.1), (64, 489, 0.2), (500, 65, 0.2), (492, 67, 0.1), (177, 177, 0.2), (250, 125, 0.1),
    (249, 125, 0.1),                                             # one pixel per frame short of the bound: 16-row tiles, separate reduction
    # column remainders 4, 8, 12, 60, 62, 63 against nrows % 32 of 0, 1, 3, 7, 8, 31, each row remainder with 5 and with 9 taps
    (196, 160, 0.1), (200, 161, 0.1), (204, 163, 0.1), (252, 167, 0.1), (254, 168, 0.1), (255, 191, 0.1),
    (196, 191, 0.2), (200, 160, 0.2), (204, 161, 0.2), (252, 163, 0.2), (254, 167, 0.2), (255, 168, 0.2),
    (208, 165, 0.2), (197, 162, 0.1), (194, 164, 0.2), (195, 166, 0.1)]]    # (beyond the issue's list: the column classes still missing)
# 32-row tiles without the reduction: subsampling 2 and 8
RB32_PLAIN = [Case("RB32_PLAIN", 180, 200, 0.1, 32, 2, 2), Case("RB32_PLAIN", 180, 200, 0.2, 32, 2, 8)]
TILED_CASES = TILED_HRED_SMALL + RB32_PLAIN

# the one launch for the gradients of every level >= 1 (batch x (levels - 1) <= 32 entries, per-entry geometry in shorts)
MERGED_GRAD = [Case("MERGED_GRAD", 300, 220, 0.1, 16, 3, 4),      # 32 entries: merged, the table is full
               Case("MERGED_GRAD", 300, 220, 0.1, 17, 3, 4),      # 34 entries: a launch per level
               Case("MERGED_GRAD", 300, 220, 0.2, 32, 2, 4),      # 32 entries of one size
               Case("MERGED_GRAD", 300, 220, 0.1, 11, 4, 2),      # 33 entries: a launch per level
               Case("MERGED_GRAD", 300, 220, 0.2, 8, 4, 2)]       # 24 entries of three sizes in one launch
BATCH_SPLIT = [Case("BATCH_SPLIT", 180, 200, 0.1, 33),            # groups of 32 and 1: the query reports the group of one frame
               Case("BATCH_SPLIT", 300, 220, 0.1, 32, kinds="mixed")]   # 16 u8 and 16 f32 frames interleaved: two groups of 16
# the two kernels that take taps of any count: seven smoothing taps; KLT_OPT_FUSED_KERNELS off
OTHER_PATHS = [Case("OTHER_PATHS", 203, 165, 0.15, 4, 3, 4), Case("OTHER_PATHS", 203, 165, 0.1, 2, 3, 4, fused=0)]
GROUPING_CASES = MERGED_GRAD + BATCH_SPLIT + OTHER_PATHS
ALL_CASES = STREAM_CASES + TILED_CASES + GROUPING_CASES


def case_path(c, f32, stream_opt=1, hreduce_opt=1):
    """expected (code, merged) of a case: its last group (a mixed case starts with a u8 frame, so its last group is the f32 one)"""
    if c.kinds == "mixed":
        return expected_path(c.ncols, c.nrows, c.batch // 2, True, c.levels, c.ss, c.sigma, stream_opt, hreduce_opt, c.fused)
    return expected_path(c.ncols, c.nrows, c.batch, f32, c.levels, c.ss, c.sigma, stream_opt, hreduce_opt, c.fused)


# ------------------------------------------------------------------------------------------------------------------------------- frames
def frames(shape, n, f32, seed):
    """`n` DISTINCT frames of `shape` = (rows, cols), so that a mix-up of the batch index shows.  u8: full-range noise over a smooth field
    (a different field and different noise per frame; both 0 and 255 occur).  f32: the same with its fractions kept, shifted to include
    negative values, plus a few runs of -0.0: a row run that reaches the last column, a column run that reaches the last row, a block in
    the frame's last corner.  No infinities (tests/test_gpu_l0_stream.py has them)."""
    rng = np.random.default_rng([int(seed), 8])
    nr, nc = shape
    y, x = np.arange(nr, dtype=np.float32), np.arange(nc, dtype=np.float32)
    out = []
    for k in range(n):
        field = np.float32(127.5) + np.float32(70) * np.outer(np.cos(y / np.float32(11.0 + k) + np.float32(0.7 * k)),
                                                              np.sin(x / np.float32(7.0 + k) + np.float32(0.3 * k))).astype(np.float32)
        noise = rng.integers(-128, 129, shape, dtype=np.int16)
        img = np.clip(field + noise, 0, 255)
        if not f32:
            out.append(img.astype(np.uint8))
            continue
        img = (img - np.float32(128.25)).astype(np.float32)
        r0, c0 = int(rng.integers(0, nr)), int(rng.integers(0, nc))
        img[r0, max(0, nc - 1 - 9 - k):] = np.float32(-0.0)
        img[max(0, nr - 1 - 5 - k):, c0] = np.float32(-0.0)
        img[nr - 3:, nc - 6:] = np.float32(-0.0)
        img[nr // 2, nc // 3:nc // 3 + 40] = np.float32(-0.0)
        out.append(img)
    return out


def case_frames(c, f32, seed=None):
    seed = c.ncols * 65536 + c.nrows if seed is None else seed
    shape = (c.nrows, c.ncols)
    if c.kinds == "mixed":
        u8, fl = frames(shape, c.batch, False, seed), frames(shape, c.batch, True, seed + 1)
        return [fl[k] if k % 2 else u8[k] for k in range(c.batch)]
    return frames(shape, c.batch, f32, seed)


# ------------------------------------------------------------------------------------------------------------------- comparison
PLANES = ("img", "gx", "gy")


def first_difference(got, want):
    """None, or a description of the first element whose BITS differ (no tolerance: +0 and -0 differ, equal NaN payloads do not)"""
    if got.shape != want.shape:
        return "shape %s against %s" % (got.shape, want.shape)
    a = np.ascontiguousarray(got, np.float32).view(np.uint32).ravel()
    b = np.ascontiguousarray(want, np.float32).view(np.uint32).ravel()
    bad = np.flatnonzero(a != b)
    if not bad.size:
        return None
    j = int(bad[0])
    ncols = got.shape[-1]
    return "%d of %d differ; first at flat index %d (row %d, column %d): got %r (0x%08x), want %r (0x%08x)" % (
        bad.size, a.size, j, j // ncols, j % ncols, got.ravel()[j], a[j], want.ravel()[j], b[j])


def oracle_pyramid(c, frame):
    from oracle import klt_oracle as ko
    return ko.Pyramids(params_from_tc(tc_of(c)), np.asarray(frame, np.float32))


def tc_of(c):
    return make_tc(levels=c.levels, ss=c.ss, smooth_sigma_fact=c.sigma)


STREAM_ORACLE_FRAMES = (0, 1, 15, 31)


def run_pyramid_trial(ctx, c, f32, oracle_frames=None, seed=None, log=None):
    """Builds the frames of case `c` in one klt_build_pyramids_batch call under every setting of KLT_OPT_L0_STREAM / KLT_OPT_FUSED_HREDUCE
    that changes the expected kernel (both on; then streaming off if the case streams, else the fused reduction off if it has one),
    asserts klt_level0_path each time, compares every plane of every level of every frame between the first build and the others, and
    the planes of every build with the oracle's for the frames in `oracle_frames` (None: all).  Returns None or a description of the
    first difference."""
    from oracle import klt_oracle as ko
    fr = case_frames(c, f32, seed)
    n = len(fr)
    settings = [(1, 1)]
    if case_path(c, f32, 0, 1) != case_path(c, f32, 1, 1):
        settings.append((0, 1))
    elif case_path(c, f32, 1, 0) != case_path(c, f32, 1, 1):
        settings.append((1, 0))
    idx = list(range(n)) if oracle_frames is None else sorted(set(k for k in oracle_frames if k < n))
    ko.set_threads(8)
    try:
        want = {k: oracle_pyramid(c, fr[k]) for k in idx}
    finally:
        ko.set_threads(1)
    ctx.configure(tc_of(c))
    first = None
    try:
        ctx.set_option(OPT_FUSED_KERNELS, c.fused)
        for stream_opt, hreduce_opt in settings:
            ctx.set_option(OPT_L0_STREAM, stream_opt)
            ctx.set_option(OPT_FUSED_HREDUCE, hreduce_opt)
            for k, f in enumerate(fr):
                ctx.upload(k, f)
            ctx.build_pyramids_batch(list(range(n)), sync=True)
            tag = "stream %d, fused reduction %d" % (stream_opt, hreduce_opt)
            got_path, want_path = ctx.level0_path(), case_path(c, f32, stream_opt, hreduce_opt)
            if log:
                log("%s: %s%s" % (tag, PATH_NAMES[got_path[0]], ", merged gradients" if got_path[1] else ""))
            if got_path != want_path:
                return "%s: klt_level0_path says %r (%s), the case was written for %r (%s)" % (
                    tag, got_path, PATH_NAMES[got_path[0]], want_path, PATH_NAMES[want_path[0]])
            planes = [[[ctx.download_level(k, p, l) for p in range(3)] for l in range(c.levels)] for k in range(n)]
            for k in range(n):
                for l in range(c.levels):
                    for p in range(3):
                        bad = None
                        if k in want:
                            bad = first_difference(planes[k][l][p], want[k].level(p, l))
                            against = "the oracle"
                        if not bad and first is not None:
                            bad = first_difference(planes[k][l][p], first[k][l][p])
                            against = "the build with both options on"
                        if bad:
                            return "%s: frame %d of %d, %s level %d against %s: %s" % (tag, k, n, PLANES[p], l, against, bad)
            if first is None:
                first = planes
    finally:
        ctx.set_option(OPT_FUSED_KERNELS, 1)
        ctx.set_option(OPT_L0_STREAM, 1)
        ctx.set_option(OPT_FUSED_HREDUCE, 1)
    return None


# ---------------------------------------------------------------------------------------------------------------------------- draws
TARGETS = ["stream", "stream", "stream", "hred", "hred", "rb32", "rb16", "rb16", "lds", "twopass"]
STREAM_MAX_PIXELS, OTHER_MAX_PIXELS = 22000000, 2000000
PYRAMID_SEEDS = [0, 1, 3, 4, 5, 6, 7, 12, 14, 16, 25, 59]       # every path code, merged and separate gradient launches (tests/test_pyramid_rule.py)


def _target_of(code):
    return {TWO_PASS: "twopass", TILED_LDS: "lds", RB16: "rb16", RB32: "rb32", RB32_HRED: "hred", STREAM: "stream", STREAM_NO_CENTRE: "stream"}[code]


def draw_pyramid(rng):
    """A Case drawn at random, with its dtype: the target kernel first (and merged or separate gradient launches), then batch (1 .. 33),
    subsampling, levels, sigma and a frame size that reach it under expected_path -- the width's and the height's remainder drawn
    uniformly from the class lists.  At most 22 M pixels per launch for the streaming kernel, 2 M for the others.  Returns (case, f32)."""
    target = TARGETS[int(rng.integers(0, len(TARGETS)))]
    want_merged = bool(rng.integers(0, 2))
    f32 = bool(rng.integers(0, 2))
    while True:                                     # (the target stays: a kernel that is harder to reach is drawn no less often)
        batch = int(rng.integers(1, 34 if target == "rb16" else 33))
        group = (batch - 1) % MAX_BATCH + 1
        sigma = 0.15 if target == "lds" else float(rng.choice([0.1, 0.2]))
        ss = 4 if target in ("stream", "hred") else int(rng.choice([2, 8])) if target == "rb32" else int(rng.choice([2, 4, 8]))
        levels = int(rng.integers(2, 5)) if ss != 8 else int(rng.integers(2, 4))
        fused = 0 if target == "twopass" else 1
        r = int(rng.choice(COL_REMAINDERS))
        if target == "stream":
            strips = int(rng.integers(2, 80))
            segs = -(-STREAM_WORKGROUPS // (strips * group))
            q = int(rng.choice(STREAM_ROW_REMAINDERS))
            ncols = STRIP * strips if r == 0 else STRIP * (strips - 1) + r
            nrows = SEG * segs if q == 0 else SEG * (segs - 1) + q
            cap = STREAM_MAX_PIXELS
        else:
            lo = TALL_PIXELS / group if target in ("hred", "rb32") else 4096
            hi = OTHER_MAX_PIXELS / min(batch, MAX_BATCH) if target in ("hred", "rb32") else min(TALL_PIXELS / group, 500000 / batch if target == "twopass" else 1e9)
            if hi <= lo:
                continue
            pixels = float(rng.uniform(lo, hi))
            aspect = float(np.exp(rng.uniform(-1.2, 1.2)))
            q = int(rng.choice(TILED_ROW_REMAINDERS))
            ncols = max(1, int(round((pixels * aspect) ** 0.5 / STRIP))) * STRIP + r
            nrows = max(2, int(round((pixels / aspect) ** 0.5 / TILE_ROWS))) * TILE_ROWS + q
            cap = OTHER_MAX_PIXELS
        coarse = ss ** (levels - 1)
        if ncols * nrows * min(batch, MAX_BATCH) > cap or ncols // coarse < 4 or nrows // coarse < 4 or ncols > 65535 or nrows > 65535 \
                or ncols * nrows >= 1 << 27:
            continue
        c = Case("DRAW", ncols, nrows, sigma, batch, levels, ss, fused)
        code, merged = case_path(c, f32)
        if _target_of(code) == target and (merged == want_merged or not fused):
            return c, f32


def drawn_case(seed):
    return draw_pyramid(np.random.default_rng([int(seed), 9]))


def draw_oracle_frames(c):
    """the frames of a drawn case that are compared with the oracle: 0, 1, 15, 31 and the last one where they exist, fewer where the frames
    are large (about 6 M pixels of oracle pyramids per trial; always frame 0)"""
    want = [k for k in (0, c.batch - 1, 1, 15, 31) if k < c.batch]
    keep = max(1, int(6000000 // (c.ncols * c.nrows)))
    return tuple(dict.fromkeys(want))[:keep]
