"""The second half of selection -- everything behind the eigenvalue keys -- at the edges of its tiles, cuts and loops: the case tables, what
the CPU oracle says each case's list is (expected_list), restatements of the host rules that only PLAN cases (expected_pick_path of
plan_selection / begin_parallel_selection / make_nms_args, expected_cut of key_bin + key_threshold_kernel + the sampled histogram; the GPU
tests assert them against klt_select_pick_path, so that drift fails instead of losing coverage), a plain restatement of the walk with four
wrong variants (walk_restated), and the trial the GPU tests run.  Scores are given (klt_set_score_override), so frame content does not
matter and a candidate map can be built to the cell.  Every comparison is exact; there is no tolerance anywhere.

Lattices: border 4 under the 7 x 7 window, so a lattice of nx x ny candidates at step s is a frame of (nx - 1) s + 9 columns."""
import collections
import functools

import numpy as np

from helpers import make_tc, params_from_tc

# ---- the constants the restatements use (test_select_pick_rule holds each against the source line it restates)
MIS_TILE, MIS_T = 32, 256
STAGE_LIMIT = 120 * 1024          # mis_stage_bytes(R) <= 120 * 1024: the parallel passes, else the serial walk
BOUND_LIMIT = 98304               # by_rank = bound <= 98304
CAND_LIMIT = 262144               # prefilter: ncand > 262144 && target < ncand / 2
TARGET_FLOOR, TARGET_PER_SLOT = 65536, 64
HIST_BINS, KEY_BIN_SHIFT = 8192, 18
NMS_T = 1024
LDS_GRID_LIMIT = 128 * 1024
RANK_GX, RANK_T = 96, 256
HIST_SAMPLE = 4                   # eigen_hist_kernel: workgroups with blockIdx.x & 3 == 0, of a grid of 1024
HIST_GRID = 1024
REPLACE_FLOOR, REPLACE_PER_SLOT = 4096, 64      # REPLACING_SOME behind the cut, parallel: max(4096, 64 * lost), in sampled units a quarter
BORDER = 4
SELECTING_ALL, REPLACING_SOME = 1, 2
OPT_PARALLEL = 8                  # KLT_OPT_SELECT_PARALLEL_NMS
BIG = 2147483520.0                # the largest f32 whose int fits
PICK_FIELDS = ("walk", "order", "cut", "attempts", "instantiation", "pass_lds", "grid", "sparse")      # asserted; passes and looks only >= 1

Entry = collections.namedtuple("Entry", "name table nx ny mindist skip form seed n mode live min_eig walks empty_ok")


def E(name, table, nx, ny, mindist, form, n, skip=0, seed=1, mode=SELECTING_ALL, live=None, min_eig=1.0, walks=(1, 0), empty_ok=False):
    return Entry(name, table, nx, ny, mindist, skip, form, seed, n, mode, live, min_eig, walks, empty_ok)


def case_id(e):
    return e.name


# ---- geometry
def frame_dims(e):
    step = e.skip + 1
    return (e.nx - 1) * step + 1 + 2 * BORDER, (e.ny - 1) * step + 1 + 2 * BORDER


def tc_of(e):
    return make_tc(mindist=e.mindist, nSkippedPixels=e.skip, min_eigenvalue=e.min_eig, borderx=BORDER, bordery=BORDER)


def radius(mindist, skip):
    d = max(mindist, 0) - 1
    return d // (skip + 1) if d >= 0 else -1


def stage_bytes(R):
    W = MIS_TILE + 2 * max(R, 0)
    return (W * MIS_TILE + W * W) * 4 if R > 0 else 0


def tile_capacity(R):
    if R < 0:
        return MIS_TILE * MIS_TILE
    per_side = (MIS_TILE + R) // (R + 1)
    return min(per_side * per_side, MIS_TILE * MIS_TILE)


def tiles_of(nx, ny):
    return -(-nx // MIS_TILE), -(-ny // MIS_TILE)


def has_interior_tile(nx, ny, R):
    """some tile whose stage (tile + halo of R cells) lies inside the lattice"""
    if R <= 0:
        return False
    tx, ty = tiles_of(nx, ny)
    return any(t * MIS_TILE - R >= 0 and t * MIS_TILE + MIS_TILE + R <= nx for t in range(tx)) and \
        any(t * MIS_TILE - R >= 0 and t * MIS_TILE + MIS_TILE + R <= ny for t in range(ty))


def bound_of(nx, ny, R):
    return nx * ny if R < 0 else -(-nx // (R + 1)) * -(-ny // (R + 1))


def target_of(n):
    return max(TARGET_FLOOR, TARGET_PER_SLOT * n)


def cut_planned(e):
    ncand = e.nx * e.ny
    return ncand > CAND_LIMIT and target_of(e.n) < ncand // 2


def parallel_walk(e, walk_opt):
    return bool(walk_opt) and e.nx * e.ny > 0 and stage_bytes(radius(e.mindist, e.skip)) <= STAGE_LIMIT


# ---- scores
def key_bins(val):
    return (np.ascontiguousarray(val, np.float32).view(np.uint32) >> KEY_BIN_SHIFT) & (HIST_BINS - 1)


def _distinct(rng, count, lo=2.0):
    """`count` distinct f32 values from lo upwards in steps of a quarter (exact in f32 below 2^22)"""
    assert lo + 0.25 * count < (1 << 22)
    return (lo + 0.25 * rng.permutation(count)).astype(np.float32)


@functools.lru_cache(maxsize=4)
def scores(e):
    """the [ny][nx] f32 score map of an entry; the same array every time (read-only)"""
    nx, ny, form = e.nx, e.ny, e.form
    rng = np.random.default_rng(e.seed)
    ys, xs = np.mgrid[0:ny, 0:nx]
    R = radius(e.mindist, e.skip)
    kind, _, arg = form.partition(":")
    if kind == "random":
        val = _distinct(rng, nx * ny).reshape(ny, nx)
    elif kind == "ties":
        val = rng.integers(1, 40, (ny, nx)).astype(np.float32) * 8.0                  # 39 distinct scores
    elif kind == "plateau":
        val = np.full((ny, nx), 50.0, np.float32)
    elif kind == "rampx":
        val = (10.0 + xs + 0.001 * ys).astype(np.float32)
    elif kind == "rampy":
        val = (10.0 + ys + 0.001 * xs).astype(np.float32)
    elif kind == "checker":
        val = np.where((xs // 3 + ys // 3) % 2 == 0, 100.0, 7.0).astype(np.float32)
    elif kind == "capacity":
        # strict maxima on a lattice of pitch R + 1 anchored at every populated tile's origin, over a valid background: the oracle
        # accepts every one of them and nothing else of their tile -- mis_tile_capacity(R) per full tile
        val = (2.0 + 40.0 * rng.random((ny, nx))).astype(np.float32)
        peak = capacity_peaks(e)
        val[peak] = _distinct(rng, int(peak.sum()), 100.0)
    elif kind == "edges":
        # random scores around the threshold with the value edges sprinkled in: exactly min_eigenvalue, the next f32 below it, exactly 1.0,
        # the largest f32 whose int fits
        val = _distinct(rng, nx * ny, max(e.min_eig - 40.0, 0.25)).reshape(ny, nx).copy()
        val[rng.random((ny, nx)) < 0.3] = 0.5                                          # a third of the map below any threshold
        spots = rng.permutation(nx * ny)[:64].reshape(4, 16)
        floor = np.float32(e.min_eig)
        assert float(floor) == e.min_eig
        for row, v in zip(spots, (floor, np.nextafter(floor, np.float32(0)), np.float32(1.0), np.float32(BIG))):
            val.reshape(-1)[row] = v
    elif kind == "thresh":
        # exactly `arg` scores pass the threshold, at random cells
        val = np.full(nx * ny, 0.5, np.float32)
        keep = rng.permutation(nx * ny)[:int(arg)]
        val[keep] = _distinct(rng, keep.size)
        val = val.reshape(ny, nx)
    elif kind == "sparse":
        # about `arg` percent of the scores pass the threshold
        val = _distinct(rng, nx * ny).reshape(ny, nx)
        val[rng.random((ny, nx)) >= float(arg) / 100.0] = 0.5
    elif kind == "blind":
        # columns 0 .. 255 random within one histogram bin, everything else far below it
        val = rng.integers(8, 2000, (ny, nx)).astype(np.float32) * 0.25               # [2, 500)
        val[:, :256] = 1024.0 + rng.integers(0, 128, (ny, 256)).astype(np.float32) * 0.25
    elif kind == "onebin":
        val = 1024.0 + rng.integers(0, 128, (ny, nx)).astype(np.float32) * 0.25
    elif kind == "twobins":
        # `arg` keys in the bin of 2048, the rest in the bin of 1024
        val = (1024.0 + rng.integers(0, 128, nx * ny) * 0.25).astype(np.float32)
        up = rng.permutation(nx * ny)[:int(arg)]
        val[up] = (2048.0 + rng.integers(0, 128, up.size) * 0.5).astype(np.float32)
        val = val.reshape(ny, nx)
    else:
        raise KeyError(form)
    val = np.ascontiguousarray(val, np.float32)
    assert np.isfinite(val).all()
    val.setflags(write=False)
    return val


def capacity_tiles_all(R):
    """True when the lattice of pitch R + 1 may fill every tile: a tile's last maximum lies more than R cells in front of the next tile"""
    per_side = (MIS_TILE + R) // (R + 1)
    return MIS_TILE - (per_side - 1) * (R + 1) > R


def capacity_peaks(e):
    R = radius(e.mindist, e.skip)
    ys, xs = np.mgrid[0:e.ny, 0:e.nx]
    peak = ((xs % MIS_TILE) % (R + 1) == 0) & ((ys % MIS_TILE) % (R + 1) == 0)
    if not capacity_tiles_all(R):
        peak &= ((xs // MIS_TILE) % 2 == 0) & ((ys // MIS_TILE) % 2 == 0)
    return peak


# ---- lists
def _oracle():
    from oracle import klt_oracle
    return klt_oracle


def empty_list(n):
    return _oracle().make_featurelist(n)


def lost_edge_slots(n):
    """lost slots first, last, and on either side of every multiple of 256"""
    idx = {0, n - 1}
    for m in range(256, n, 256):
        idx.update((m - 1, m))
    return np.array(sorted(i for i in idx if 0 <= i < n))


@functools.lru_cache(maxsize=4)
def list_in(e):
    """the list a REPLACING_SOME entry starts from (None for SELECTING_ALL): e.live names the kind"""
    if e.mode == SELECTING_ALL:
        return None
    nc, nr = frame_dims(e)
    d = max(e.mindist, 0) - 1
    step = e.skip + 1
    x_last, y_last = BORDER + (e.nx - 1) * step, BORDER + (e.ny - 1) * step
    rng = np.random.default_rng(e.seed + 1000)
    fl = empty_list(e.n)
    kind, _, arg = e.live.partition(":")

    def put(i, x, y, val=0):
        fl["x"][i], fl["y"][i], fl["val"][i] = x, y, val

    if kind == "fixed":
        # live features at the fractional parts .0 / .49 / .5 / .51, in the first and last candidate column and row, within d of the frame
        # edge, in the border margin outside the lattice, and with overlapping squares; `arg` slots of the rest are lost ("all": every slot)
        cx, cy = nc // 2, nr // 2
        spots = [(cx + 0.0, cy + 0.0), (cx + 30.49, cy + 0.49), (cx - 30.5, cy + 0.5), (cx + 0.51, cy - 30.51),
                 (BORDER, cy - 17), (x_last, cy + 17), (cx - 17, BORDER), (cx + 17, y_last), (BORDER + 0.51, BORDER + 0.49),
                 (x_last + 0.5, y_last + 0.5),
                 (min(d, nc - 1), cy + 40), (nc - 1 - min(d, nc - 1) + 0.5, cy - 40), (cx + 40, min(d, nr - 1)), (cx - 40, nr - 1 - min(d, nr - 1)),
                 (0.0, 0.0), (1.49, nr - 1), (nc - 1, 2.51), (nc - 1 + 0.49, nr - 1 + 0.49), (BORDER - 1, cy), (cx, BORDER - 0.51),
                 (cx + 60, cy + 20), (cx + 60 + max(d, 1), cy + 20), (cx + 61, cy + 20 + max(d, 1) // 2), (cx + 60, cy + 20)]
        assert e.n > len(spots)
        for i, (x, y) in enumerate(spots):
            put(2 * i + 1 if 2 * i + 1 < e.n else i, float(np.clip(x, 0, nc - 0.01)), float(np.clip(y, 0, nr - 0.01)), 3 + i)
        if arg == "all":
            fl["val"], fl["x"], fl["y"] = -1, -1, -1
        else:
            free = np.flatnonzero(fl["val"] < 0)
            keep_lost = int(arg)
            assert keep_lost <= free.size
            fill = free if keep_lost == 0 else np.delete(free, rng.permutation(free.size)[:keep_lost])
            for i in fill:                                  # the other slots: live features at random positions
                put(i, rng.uniform(0, nc - 1), rng.uniform(0, nr - 1), 1)
    elif kind == "long":
        # a long list: every slot live at a random position, except the lost slots at the list's edges and at every multiple of 256
        fl["x"] = rng.uniform(0, nc - 1, e.n).astype(np.float32)
        fl["y"] = rng.uniform(0, nr - 1, e.n).astype(np.float32)
        fl["val"] = rng.integers(0, 9, e.n)
        lost = lost_edge_slots(e.n)
        fl["val"][lost], fl["x"][lost], fl["y"][lost] = -1, -1, -1
    elif kind == "lost":
        # `arg` lost slots at random places of a list whose other slots are live at random positions
        fl["x"] = rng.uniform(0, nc - 1, e.n).astype(np.float32)
        fl["y"] = rng.uniform(0, nr - 1, e.n).astype(np.float32)
        fl["val"] = 0
        lost = rng.permutation(e.n)[:int(arg)]
        fl["val"][lost], fl["x"][lost], fl["y"][lost] = -1, -1, -1
    else:
        raise KeyError(e.live)
    fl.setflags(write=False)
    return fl


def oracle_list(e, val):
    """the oracle's list over the score map `val`: ko.sorted_candidates + ko.enforce_min_distance"""
    ko = _oracle()
    nc, nr = frame_dims(e)
    p = params_from_tc(tc_of(e))
    bx, by, _, _ = ko.scan_borders(p)
    assert (bx, by) == (BORDER, BORDER)
    cand = ko.sorted_candidates(val, nc, nr, bx, by, p.nSkippedPixels)
    fl = list_in(e)
    out = ko.make_featurelist(e.n) if fl is None else fl.copy()
    ko.enforce_min_distance(cand, out, nc, nr, p.mindist, p.min_eigenvalue, fl is None)
    return out


@functools.lru_cache(maxsize=4)
def expected_list(e):
    out = oracle_list(e, scores(e))
    out.setflags(write=False)
    return out


def free_slots(e):
    fl = list_in(e)
    return e.n if fl is None else int((fl["val"] < 0).sum())


def placed_count(e, out):
    """what klt_select reports: the free slots that were filled"""
    fl = list_in(e)
    return int((out["val"] >= 0).sum()) if fl is None else int(((fl["val"] < 0) & (out["val"] >= 0)).sum())


# ---- the cut
def live_blocked(e):
    """[ny][nx] bool: candidates inside the square of a live feature (REPLACING_SOME; seed_fill_kernel)"""
    blocked = np.zeros((e.ny, e.nx), bool)
    fl = list_in(e)
    d = max(e.mindist, 0) - 1
    if fl is None or d < 0:
        return blocked
    nc, nr = frame_dims(e)
    pix = np.zeros((nr, nc), bool)
    for f in fl[fl["val"] >= 0]:
        cx, cy = int(f["x"]), int(f["y"])
        pix[max(cy - d, 0):max(cy + d + 1, 0), max(cx - d, 0):max(cx + d + 1, 0)] = True
    step = e.skip + 1
    return pix[BORDER:BORDER + (e.ny - 1) * step + 1:step, BORDER:BORDER + (e.nx - 1) * step + 1:step]


def expected_cut(keys, target, sampled):
    """(threshold bin, valid keys below it) of the top-K cut over `keys` ([ny][nx] f32 scores, 0 where the candidate has no key) aiming at
    `target` kept keys: key_bin, the suffix rule of key_threshold_kernel, and -- sampled -- the histogram of eigen_hist_kernel, which sees
    the 256-key blocks whose index is 0 mod 4 and compares with a quarter of the target"""
    flat = np.ascontiguousarray(keys, np.float32).reshape(-1)
    valid = flat != 0
    bins = key_bins(flat)
    seen = valid
    if sampled:
        assert -(-flat.size // 256) >= HIST_GRID, "the grid of eigen_hist_kernel is clamped to 1024 workgroups only from 1024 blocks on"
        seen = valid & ((np.arange(flat.size) // 256) % HIST_SAMPLE == 0)
        target = (target + HIST_SAMPLE - 1) // HIST_SAMPLE
    hist = np.bincount(bins[seen], minlength=HIST_BINS)
    suffix = np.cumsum(hist[::-1])[::-1]                    # suffix[b] = keys in bins >= b
    if suffix[0] < target:
        return 0, 0
    thr = int(np.flatnonzero(suffix >= target).max())       # the largest bin that still leaves `target` keys at or above it
    return thr, int((valid & (bins < thr)).sum())


def cut_of(e, parallel):
    """(keys of the entry as the cut sees them, threshold bin, dropped) -- the planned cut of this entry on either walk"""
    val = scores(e)
    keys = np.where((val.astype(np.float64) >= max(e.min_eig, 1.0)) & ~live_blocked(e), val, np.float32(0))
    if parallel and e.mode == REPLACING_SOME:
        target = max(REPLACE_FLOOR, REPLACE_PER_SLOT * free_slots(e))      # sized by the lost slots (key_threshold_kernel reads their number)
    else:
        target = target_of(e.n)
    thr, dropped = expected_cut(keys, target, sampled=parallel)
    return keys, thr, dropped


@functools.lru_cache(maxsize=None)
def expected_attempts(e, parallel):
    """2 when the cut is planned, drops a valid key, and what it keeps does not fill the list (the oracle over the kept keys says)"""
    if not cut_planned(e):
        return 1
    keys, thr, dropped = cut_of(e, parallel)
    if dropped == 0:
        return 1
    kept = np.where(key_bins(keys) >= thr, keys, np.float32(0))
    return 2 if placed_count(e, oracle_list(e, kept)) < free_slots(e) else 1


def expected_pick_path(e, walk_opt):
    """klt_select_pick_path after the entry's selection under KLT_OPT_SELECT_PARALLEL_NMS = walk_opt: plan_selection,
    begin_parallel_selection and make_nms_args restated (passes and looks are not planned)"""
    R = radius(e.mindist, e.skip)
    parallel = parallel_walk(e, walk_opt)
    cut = cut_planned(e)
    attempts = expected_attempts(e, parallel)
    if parallel:
        by_rank = bound_of(e.nx, e.ny, R) <= BOUND_LIMIT
        lds = stage_bytes(R) + ((tile_capacity(R) * 2 + 15) & ~15)
        sparse = int(e.mode == REPLACING_SOME and cut and attempts == 1)        # (the repeat with every candidate is dense)
        return dict(walk=1, order=1 if by_rank else 2, cut=int(cut), attempts=attempts, instantiation=9 if R == 9 else 0, pass_lds=lds,
                    grid=0, sparse=sparse)
    nc, nr = frame_dims(e)
    return dict(walk=0, order=0, cut=int(cut), attempts=attempts, instantiation=0, pass_lds=0,
                grid=0 if walk_grid_in_lds(nc, nr, e.mindist) else 1, sparse=0)


def walk_grid_in_lds(ncols, nrows, mindist):
    d = max(mindist, 0) - 1
    cell = d + 1 if d >= 0 else 1
    gw, gh = (-(-ncols // cell), -(-nrows // cell)) if d >= 0 else (1, 1)
    return gw * gh * 4 <= LDS_GRID_LIMIT


# ---- a plain restatement of the walk, with four wrong variants
MUTANTS = ("strict_square", "ties_left_first", "ties_up_first", "slots_reversed")


def walk_restated(e, mutant=None, val=None):
    """_enforceMinimumDistance (selectGoodFeatures.py:45-135) over the entry's scores in plain numpy / Python.  mutant: None, or one of
    MUTANTS -- `<` for `<=` in the square test, equal scores ranked left before right, equal scores in a column ranked up before down, the
    free slots taken in another order than list order."""
    assert mutant is None or mutant in MUTANTS
    val = scores(e) if val is None else val
    nc, nr = frame_dims(e)
    step = e.skip + 1
    d = max(e.mindist, 0) - 1
    yi, xi = np.nonzero(val.astype(np.float64) >= max(e.min_eig, 1.0))
    v = val[yi, xi]
    x, y = BORDER + xi * step, BORDER + yi * step
    # rank: value, then x, then y, all descending
    order = np.lexsort((y if mutant == "ties_up_first" else -y, x if mutant == "ties_left_first" else -x, -v.astype(np.float64)))
    fl = list_in(e)
    out = empty_list(e.n) if fl is None else fl.copy()
    taken = np.zeros((nr, nc), bool)
    reach = d - 1 if mutant == "strict_square" else d

    def mark(cx, cy, r):
        if r >= 0:
            taken[max(cy - r, 0):max(cy + r + 1, 0), max(cx - r, 0):max(cx + r + 1, 0)] = True

    if fl is not None:
        for f in fl[fl["val"] >= 0]:
            mark(int(f["x"]), int(f["y"]), reach)
        slots = np.flatnonzero(fl["val"] < 0)
    else:
        slots = np.arange(e.n)
    if mutant == "slots_reversed":
        slots = slots[::-1]
    k = 0
    for j in order:
        if k >= slots.size:
            break
        cx, cy = int(x[j]), int(y[j])
        if taken[cy, cx]:
            continue
        out[slots[k]] = (cx, cy, int(v[j]), 0)
        k += 1
        mark(cx, cy, reach)
    return out


def lists_difference(got, want):
    """None, or where two lists differ first: x, y and val of every slot, bit for bit"""
    if got.shape != want.shape:
        return "shape %r, want %r" % (got.shape, want.shape)
    bad = np.flatnonzero((got["x"] != want["x"]) | (got["y"] != want["y"]) | (got["val"] != want["val"]))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d of %d slots differ; first slot %d: got (%r, %r, %d), want (%r, %r, %d)" % (
        bad.size, got.size, i, got["x"][i], got["y"][i], got["val"][i], want["x"][i], want["y"][i], want["val"][i])


# ---- the tables
RADII = (-1, 0, 1, 3, 4, 8, 9, 10, 16, 17, 31, 32, 48, 49, 63, 64, 65)
CAPACITY_RADII = (0, 1, 2, 15, 31)
FORMS = ("random", "ties", "plateau", "rampx", "rampy", "checker")


def _interior_lattice(R):
    """the smallest whole-tile lattice side with an interior tile at radius R"""
    return MIS_TILE * (2 * -(-max(R, 0) // MIS_TILE) + 1)


def _passes():
    t = []
    for k, R in enumerate(RADII):
        # one lattice with no interior tile (sides 0, 1 or 31 past a tile edge), one with at least one
        rx, ry = ((0, 1), (1, 31), (31, 0))[k % 3]
        small_x, small_y = (64 + rx if R < 17 else 33), (32 + ry if ry else 64)
        side = _interior_lattice(R)
        t.append(E("R%d_edge_%dx%d" % (R, small_x, small_y), "PASSES", small_x, small_y, R + 1, FORMS[k % 6], 300, seed=10 + k))
        t.append(E("R%d_interior_%dx%d" % (R, side + ry, side + rx), "PASSES", side + ry, side + rx, R + 1, FORMS[(k + 1) % 6], 300, seed=40 + k))
    t += [E("R9_skip1_mindist19", "PASSES", 97, 96, 19, "random", 300, skip=1, seed=70),
          E("R9_skip1_mindist20", "PASSES", 96, 127, 20, "ties", 300, skip=1, seed=71)]
    # tile counts 1 / 7 / 8 / 9 / 17, one tile row, one tile column: fewer than the 8 XCDs, exactly 8, and remainders
    for name, nx, ny in (("tiles1", 31, 32), ("tiles7", 7 * 32, 31), ("tiles8", 8 * 32 - 31, 32), ("tiles9", 65, 96), ("tiles17", 17 * 32 - 1, 8),
                         ("tilerow", 5 * 32, 33 - 1), ("tilecol", 8, 5 * 32 + 1), ("tilecol32", 32, 3 * 32 + 31)):
        t.append(E("%s_%dx%d" % (name, nx, ny), "PASSES", nx, ny, 4, "random", 200, seed=80 + len(t)))
    # every score form at the compiled-in radius and at the narrow loop, on a lattice with interior tiles; the ramps are dependency
    # chains of nx / (R + 1) and ny / (R + 1) passes
    for k, form in enumerate(FORMS):
        t.append(E("form_%s_R9" % form, "PASSES", 129, 97, 10, form, 250, seed=100 + k))
        t.append(E("form_%s_R1" % form, "PASSES", 97, 129, 2, form, 5000, seed=110 + k))
    t += [E("chain_rampx_R1_200", "PASSES", 200, 40, 2, "rampx", 3000, seed=120), E("chain_rampy_R4_300", "PASSES", 40, 300, 5, "rampy", 600, seed=121)]
    # a tile filled to exactly its capacity
    for R in CAPACITY_RADII:
        t.append(E("capacity_R%d" % R, "PASSES", 96 + (R == 2) * 32, 64 + (R == 2) * 64 + 5, R + 1, "capacity", 20000, seed=130 + R))
    # value edges: scores at the threshold, one f32 below it, 1.0, the largest f32 whose int fits
    t += [E("values_min_eig_1", "PASSES", 70, 65, 4, "edges", 400, seed=140), E("values_min_eig_37.5", "PASSES", 65, 70, 4, "edges", 400, seed=141, min_eig=37.5),
          E("values_min_eig_37.5_R0", "PASSES", 65, 70, 1, "edges", 5000, seed=142, min_eig=37.5)]
    # ordering: a bound of exactly 98304 is ranked by counting, one column more is sorted and walked
    for mindist in (1, 0):
        t.append(E("rank_384x256_mindist%d" % mindist, "PASSES", 384, 256, mindist, "sparse:20", 3000, seed=150 + mindist))
        t.append(E("sort_385x256_mindist%d" % mindist, "PASSES", 385, 256, mindist, "sparse:20", 3000, seed=152 + mindist))
    # accepted counts either side of 96 chunks of 256 keys, and far beyond, against list lengths around them
    t += [E("accepted_24576_n_a", "PASSES", 256, 256, 1, "thresh:24576", 24576, seed=160),
          E("accepted_24576_n_a-1", "PASSES", 256, 256, 1, "thresh:24576", 24575, seed=160),
          E("accepted_24577_n_a+1", "PASSES", 256, 256, 1, "thresh:24577", 24578, seed=161),
          E("accepted_24577_n_1", "PASSES", 256, 256, 1, "thresh:24577", 1, seed=161),
          E("accepted_60000_n_4a", "PASSES", 256, 256, 1, "thresh:60000", 240000, seed=162),
          E("accepted_300_n_255", "PASSES", 100, 70, 1, "thresh:300", 255, seed=163), E("accepted_256_n_256", "PASSES", 100, 70, 1, "thresh:256", 256, seed=164),
          E("accepted_256_n_257", "PASSES", 100, 70, 1, "thresh:256", 257, seed=165), E("accepted_none", "PASSES", 100, 70, 4, "thresh:0", 10, seed=166, empty_ok=True)]
    # more than 4096 tiles: the 16-deep unrolled trips of mis_compact_kernel
    t.append(E("tiles4160_2049x2048", "PASSES", 2049, 2048, 10, "sparse:3", 5000, seed=170))
    return t


def _replace():
    t = []
    for skip in (0, 1):
        for lost in ("0", "1", "9", "all"):
            t.append(E("fixed_lost%s_skip%d" % (lost, skip), "REPLACE", 150, 120, 10 + skip, "random", 60, skip=skip, seed=200 + len(t), mode=REPLACING_SOME,
                       live="fixed:" + lost, empty_ok=lost == "0"))
        t.append(E("fixed_lost9_ties_skip%d" % skip, "REPLACE", 131, 97, 4, "ties", 70, skip=skip, seed=210 + skip, mode=REPLACING_SOME, live="fixed:9"))
    for n in (255, 256, 257, 4095, 4096, 4097, 8193):
        t.append(E("long_%d" % n, "REPLACE", 300, 200, 2, "random", n, seed=220 + len(t), mode=REPLACING_SOME, live="long"))
    t.append(E("long_8193_mindist0", "REPLACE", 300, 200, 0, "random", 8193, seed=240, mode=REPLACING_SOME, live="long"))
    t.append(E("lost_half_of_9000", "REPLACE", 300, 200, 2, "random", 9000, seed=241, mode=REPLACING_SOME, live="lost:4500"))
    return t


def _cut():
    t = [E("nocut_512x512", "CUT", 512, 512, 10, "random", 500, seed=300),
         E("cut_512x513_holds", "CUT", 512, 513, 10, "random", 500, seed=301),
         E("cut_n2051_below_half", "CUT", 512, 513, 3, "random", 2051, seed=302),
         E("nocut_n2052_at_half", "CUT", 512, 513, 3, "random", 2052, seed=303),
         E("nocut_n2053_above_half", "CUT", 512, 513, 3, "random", 2053, seed=304),
         E("cut_n1024", "CUT", 512, 513, 6, "random", 1024, seed=305), E("cut_n1025", "CUT", 512, 513, 6, "random", 1025, seed=306),
         E("cut_few_valid", "CUT", 512, 513, 6, "thresh:30000", 1000, seed=307),
         E("cut_one_bin", "CUT", 512, 513, 10, "onebin", 1000, seed=308),
         E("cut_two_bins_target-1", "CUT", 512, 513, 4, "twobins:65535", 1024, seed=309),
         E("cut_two_bins_target", "CUT", 512, 513, 4, "twobins:65536", 1024, seed=310),
         E("cut_two_bins_target+1", "CUT", 512, 513, 4, "twobins:65537", 1024, seed=311),
         E("cut_two_bins_runs_out", "CUT", 512, 513, 26, "twobins:65536", 1024, seed=312),
         E("cut_runs_out", "CUT", 512, 513, 26, "random", 2000, seed=313),
         E("sample_blind", "CUT", 1024, 300, 10, "blind", 2000, seed=314)]
    # REPLACING_SOME behind the cut (sparse passes: four tiles per workgroup, 272 tiles = 34 per XCD, no multiple of 4); 240 live features
    for lost in (1, 64, 65, 1000):
        t.append(E("cut_replace_lost%d" % lost, "CUT", 512, 513, 10, "random", lost + 240, seed=320 + len(t), mode=REPLACING_SOME, live="lost:%d" % lost))
    t.append(E("cut_replace_runs_out", "CUT", 512, 513, 26, "random", 1010, seed=330, mode=REPLACING_SOME, live="lost:1000"))
    return t


PASSES, REPLACE, CUT = _passes(), _replace(), _cut()
ALL_ENTRIES = PASSES + REPLACE + CUT
DRAW_SEEDS = (3, 11, 19, 23, 42, 57, 64, 77, 81, 90, 101, 113)


def draw_entry(seed):
    """a drawn lattice, radius, score form, mode and list length from the classes of the tables"""
    rng = np.random.default_rng(seed)
    R = int(rng.choice(RADII))
    skip = int(rng.integers(0, 2)) if R >= 0 else 0
    side = _interior_lattice(R) if rng.random() < 0.5 else 33
    nx, ny = side + int(rng.choice([0, 1, 31])) + 32 * int(rng.integers(0, 2)), side + int(rng.choice([0, 1, 31]))
    mindist = R * (skip + 1) + 1 + int(rng.integers(0, skip + 1)) if R >= 0 else 0
    form = str(rng.choice(FORMS + ("sparse:30", "edges")))
    n = int(rng.choice([1, 255, 256, 257, 1500]))
    if rng.random() < 0.4:                                  # a dozen live features, the other slots lost (a large square may block every candidate)
        return E("draw%d" % seed, "DRAW", nx, ny, mindist, form, n + 12, skip=skip, seed=seed, mode=REPLACING_SOME, live="lost:%d" % n,
                 empty_ok=True)
    return E("draw%d" % seed, "DRAW", nx, ny, mindist, form, n, skip=skip, seed=seed)


# ---- klt_min_distance_walk on its own, against oracle/min_distance_walk.py
Walk = collections.namedtuple("Walk", "name ncols nrows mindist overwrite n keys live")


def pack_keys(val, x, y):
    return (np.asarray(val, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.asarray(x, np.uint64) << np.uint64(16)) \
        | np.asarray(y, np.uint64)


def _points(rng, count, ncols, nrows, distinct=True):
    """`count` candidates (val, x, y) at random pixels, in random (not sorted) order"""
    if distinct:
        cells = rng.choice(ncols * nrows, count, replace=False) if ncols * nrows < (1 << 22) else None
        if cells is None:
            x, y = rng.integers(0, ncols, count), rng.integers(0, nrows, count)
        else:
            x, y = cells % ncols, cells // ncols
    else:
        x, y = rng.integers(0, ncols, count), rng.integers(0, nrows, count)
    val = (1.0 + rng.integers(0, 4000, count) * 0.5).astype(np.float32)
    return val, np.asarray(x, np.int64), np.asarray(y, np.int64)


def _walks():
    t = []
    rng = np.random.default_rng(500)
    for nkeys in (0, 1, 1023, 1024, 1025, 2049):
        t.append(Walk("nkeys%d" % nkeys, 300, 200, 3, 1, 4000, _points(rng, nkeys, 300, 200), None))
    # more than 64 survivors in one super-batch: 200 candidates 20 pixels apart, all accepted, then a candidate next to number 110 (blocked by
    # the grid re-test of a later batch of 64 survivors) and one next to number 130 in the same batch of 64 (blocked by the register compare)
    gx, gy = np.meshgrid(np.arange(20) * 20 + 5, np.arange(10) * 20 + 5)
    x, y = gx.reshape(-1), gy.reshape(-1)
    x = np.concatenate([x[:131], [x[130] + 9], x[131:], [x[110] - 9, x[3] + 10]])
    y = np.concatenate([y[:131], [y[130] - 9], y[131:], [y[110] + 9, y[3]]])
    t.append(Walk("survivors_beyond_lane63", 420, 220, 10, 1, 500, (np.linspace(900, 100, x.size).astype(np.float32), x, y), None))
    # the list fills up on the last key of a super-batch, and on the first of the next (mindist 1: distinct pixels never exclude each other)
    pts = _points(rng, 2049, 300, 200)
    t.append(Walk("full_on_last_key_of_batch", 300, 200, 1, 1, 1024, pts, None))
    t.append(Walk("full_on_first_key_of_batch", 300, 200, 1, 1, 1025, pts, None))
    t.append(Walk("mindist0_fewer_slots", 300, 200, 0, 1, 100, _points(rng, 500, 300, 200, distinct=False), None))
    # the cell grid in LDS (32768 cells) and in global memory (one column of cells more); some pixels occur twice
    for ncols, nrows, mindist in ((256, 128, 1), (257, 128, 1), (2560, 1280, 10), (2570, 1280, 10)):
        t.append(Walk("grid_%dx%d_mindist%d" % (ncols, nrows, mindist), ncols, nrows, mindist, 1, 3000, _points(rng, 1500, ncols, nrows, distinct=False), None))
    # cell sizes with coordinates up to 65534 on either axis (the two smallest cells on strips: their grids over 65535 x 65535 take GiB)
    for mindist in (2, 3, 7, 11, 100, 255, 256, 257):
        shapes = ((65535, 600), (600, 65535)) if mindist < 7 else ((65535, 65535),)
        for ncols, nrows in shapes:
            count = 300 if mindist <= 11 else 10       # (the plain-Python oracle marks every pixel of a square)
            val, x, y = _points(rng, count, ncols, nrows)
            if count > 100:                                 # the second half: each next to a point of the first, up to one pixel past the square
                half = count // 2
                x[half:] = np.clip(x[:count - half] + rng.integers(-mindist, mindist + 1, count - half), 0, ncols - 1)
                y[half:] = np.clip(y[:count - half] + rng.integers(-mindist, mindist + 1, count - half), 0, nrows - 1)
            x[:4], y[:4] = (ncols - 1, ncols - 1, 0, max(ncols - 1 - (mindist - 1), 0)), (nrows - 1, 0, nrows - 1, nrows - 1)
            if mindist > 11:                                # a cluster around one point: inside, on and just outside the square's edge
                x[4:10] = 30000 + np.array([0, mindist - 1, mindist, -(mindist - 1), 2 * mindist - 1, 2 * mindist - 2]) * (ncols > 60000)
                y[4:10] = 300 + np.array([0, 0, 0, mindist - 1, 0, 1])
            t.append(Walk("mindist%d_%dx%d" % (mindist, ncols, nrows), ncols, nrows, mindist, 1, 400, (val, x, y), None))
    # kept lists longer than 1024 slots: the candidates inside the live squares are the caller's to drop
    for n in (1025, 3000):
        live = empty_list(n)
        keep = np.flatnonzero(rng.random(n) < 0.5)
        live["x"][keep], live["y"][keep], live["val"][keep] = rng.uniform(0, 299, keep.size), rng.uniform(0, 199, keep.size), 5
        val, x, y = _points(rng, 3000, 300, 200)
        d = 2
        lx, ly = live["x"][keep].astype(np.int64), live["y"][keep].astype(np.int64)
        inside = ((np.abs(x[:, None] - lx[None, :]) <= d) & (np.abs(y[:, None] - ly[None, :]) <= d)).any(axis=1)
        t.append(Walk("kept_list_%d" % n, 300, 200, 3, 0, n, (val[~inside], x[~inside], y[~inside]), live))
    return t


WALK = _walks()


def walk_expected(w):
    """oracle/min_distance_walk.py over the case's candidates in the given order"""
    from oracle.min_distance_walk import enforce_minimum_distance
    val, x, y = w.keys
    fl = empty_list(w.n) if w.live is None else w.live.copy()
    feats = [[float(f["x"]), float(f["y"]), int(f["val"])] for f in fl]
    enforce_minimum_distance([(float(v), int(a), int(b)) for v, a, b in zip(val, x, y)], feats, w.ncols, w.nrows, w.mindist, 1.0, bool(w.overwrite))
    out = empty_list(w.n)
    for i, (fx, fy, fv) in enumerate(feats):
        out[i] = (fx, fy, fv, 0)
    return out


# ---- the trials the GPU tests run
_FRAMES = {}


def _frame(nc, nr):
    if (nc, nr) not in _FRAMES:
        _FRAMES.clear()
        _FRAMES[nc, nr] = np.zeros((nr, nc), np.uint8)      # the scores are given: the pixels only have to be there
    return _FRAMES[nc, nr]


def run_pick_trial(ctx, e, slot=2):
    """The entry's selection under each walk option of e.walks: None, or what differs first -- the list, the placed count, or
    klt_select_pick_path against expected_pick_path.  Prints passes and looks (they depend on the passes the previous selection needed and
    on scheduling: reported, asserted only as at least 1)."""
    want = expected_list(e)
    val = scores(e)
    fl = list_in(e)
    nc, nr = frame_dims(e)
    ctx.configure(tc_of(e))
    ctx.upload(slot, _frame(nc, nr))
    try:
        for walk in e.walks:
            ctx.set_option(OPT_PARALLEL, walk)
            ctx.set_score_override(val)
            got, placed = ctx.select(slot, e.n) if fl is None else ctx.select(slot, e.n, mode=REPLACING_SOME, fl=fl)
            tag = "%s, KLT_OPT_SELECT_PARALLEL_NMS %d" % (e.name, walk)
            bad = lists_difference(got, want)
            if bad:
                return "%s: %s" % (tag, bad)
            if placed != placed_count(e, want):
                return "%s: placed %d, want %d" % (tag, placed, placed_count(e, want))
            path, plan = ctx.select_pick_path(), expected_pick_path(e, walk)
            print("pick %s walk %d passes %d looks %d" % (e.name, path["walk"], path["passes"], path["looks"]))
            if {k: path[k] for k in PICK_FIELDS} != plan:
                return "%s: klt_select_pick_path says %r, the case was written for %r" % (tag, path, plan)
            if (path["passes"] >= 1, path["looks"] >= 1) != (plan["walk"] == 1,) * 2:
                return "%s: %d passes and %d looks on walk %d" % (tag, path["passes"], path["looks"], plan["walk"])
    finally:
        ctx.set_option(OPT_PARALLEL, 1)
    return None


def run_walk_trial(ctx, w):
    val, x, y = w.keys
    fl = empty_list(w.n) if w.live is None else w.live
    got, placed = ctx.min_distance_walk(pack_keys(val, x, y), w.ncols, w.nrows, w.mindist, w.overwrite, fl)
    want = walk_expected(w)
    bad = lists_difference(got, want)
    if bad:
        return "%s: %s" % (w.name, bad)
    want_placed = int((want["val"] >= 0).sum()) - (0 if w.live is None else int((w.live["val"] >= 0).sum()))
    if placed != want_placed:
        return "%s: placed %d, want %d" % (w.name, placed, want_placed)
    return None
