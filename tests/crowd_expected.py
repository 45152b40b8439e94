"""TEST INFRASTRUCTURE ONLY -- the crowding check's rule (include/klt_gpu.h, "crowding check") in plain numpy /
Python, as the header states it: the serial walk, the parallel-rounds form the kernels use, and the lists the tests run both on."""
import numpy as np

KLT_TRACKED = 0
KLT_CROWDED = -10
INT32_MAX = 0x7FFFFFFF
FEAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("val", np.int32), ("aux", np.int32)])
CROWD_DTYPE = np.dtype([("age", np.int32), ("winner", np.int32), ("val", np.int32), ("pad", np.int32)])


def records(x, y, val=0, aux=0):
    fl = np.zeros(len(x), FEAT_DTYPE)
    fl["x"], fl["y"], fl["val"], fl["aux"] = x, y, val, aux
    return fl


def crowd_records(age):
    prev = np.zeros(len(age), CROWD_DTYPE)
    prev["age"] = age
    return prev


def candidate_mask(out, ncols, nrows):
    """step 1: f32 comparisons, NaN and the infinities fail, -0.0 passes"""
    x, y = out["x"], out["y"]
    with np.errstate(invalid="ignore"):
        return (out["val"] == KLT_TRACKED) & (x >= np.float32(0)) & (x < np.float32(ncols)) & (y >= np.float32(0)) & (y < np.float32(nrows))


def pixels(out, cand):
    """truncation, of candidates only (the others may hold anything)"""
    px, py = np.zeros(len(out), np.int64), np.zeros(len(out), np.int64)
    px[cand], py[cand] = out["x"][cand].astype(np.int64), out["y"][cand].astype(np.int64)
    return px, py


def ages_in(prev, n):
    """step 2"""
    if prev is None:
        return np.zeros(n, np.int64)
    return np.maximum(np.asarray(prev["age"], np.int64), 0)


def priority_order(cand, age):
    """step 3: the candidates' record numbers by age descending, then index ascending"""
    idx = np.flatnonzero(cand)
    return idx[np.lexsort((idx, -age[idx]))]


def serial_walk(px, py, order, r):
    """step 4: {record: -1 kept | the winner's record number}, by the walk itself -- every candidate against the kept ones before it"""
    kept = np.zeros(len(order), np.int64)                    # record numbers of the kept ones, in the order they were kept
    kx, ky = np.zeros(len(order), np.int64), np.zeros(len(order), np.int64)
    nk = 0
    verdict = {}
    for i in order:
        covering = (np.abs(kx[:nk] - px[i]) <= r) & (np.abs(ky[:nk] - py[i]) <= r)
        if covering.any():
            verdict[int(i)] = int(kept[np.argmax(covering)])         # the first kept one that covers it
        else:
            verdict[int(i)] = -1
            kept[nk], kx[nk], ky[nk] = i, px[i], py[i]
            nk += 1
    return verdict


def crowd_check_expected(out, prev, ncols, nrows, min_distance):
    """-> (out', crowd): steps 1 to 5"""
    out = np.array(out, FEAT_DTYPE)
    n, r = len(out), min_distance - 1
    cand = candidate_mask(out, ncols, nrows)
    px, py = pixels(out, cand)
    age = ages_in(prev, n)
    verdict = serial_walk(px, py, priority_order(cand, age), r)
    crowd = np.zeros(n, CROWD_DTYPE)
    crowd["winner"] = -1
    for i, w in verdict.items():
        if w < 0:
            crowd[i] = (min(int(age[i]), INT32_MAX - 1) + 1, -1, 1, 0)
        else:
            crowd[i] = (0, w, 2, 0)
            out[i] = (-1.0, -1.0, KLT_CROWDED, out["aux"][i])
    return out, crowd


def parallel_rounds(px, py, order, r):
    """the form the kernels use, in synchronous rounds (every decision of a round reads the states the round began with): kept, if every
    higher-priority neighbour is crowded; crowded, if any higher-priority neighbour is kept; until none is undecided.
    -> ({record: True kept | False crowded}, rounds)"""
    rank = {int(i): k for k, i in enumerate(order)}
    order = [int(i) for i in order]
    higher = {i: [j for j in order if rank[j] < rank[i] and abs(px[i] - px[j]) <= r and abs(py[i] - py[j]) <= r] for i in order} \
        if len(order) <= 400 else None
    if higher is None:                                       # (long lists: neighbours through a grid of r + 1 pixel cells)
        cell = {}
        s = r + 1
        for i in order:
            cell.setdefault((px[i] // s, py[i] // s), []).append(i)
        higher = {}
        for i in order:
            cx, cy = px[i] // s, py[i] // s
            higher[i] = [j for dy in (-1, 0, 1) for dx in (-1, 0, 1) for j in cell.get((cx + dx, cy + dy), ())
                         if rank[j] < rank[i] and abs(px[i] - px[j]) <= r and abs(py[i] - py[j]) <= r]
    state = {}
    rounds = 0
    while len(state) < len(order):
        new = {}
        for i in order:
            if i in state:
                continue
            if any(state.get(j) is True for j in higher[i]):
                new[i] = False
            elif all(state.get(j) is False for j in higher[i]):
                new[i] = True
        assert new, "a round must decide the first undecided candidate of the order"
        state.update(new)
        rounds += 1
    return state, rounds


def live_pairs_within(fl, r, ncols, nrows):
    """the number of pairs of live records (val >= 0, inside the frame) whose pixels are within r of each other in x and in y"""
    live = (fl["val"] >= 0) & (fl["x"] >= 0) & (fl["x"] < ncols) & (fl["y"] >= 0) & (fl["y"] < nrows)
    px, py = fl["x"][live].astype(np.int64), fl["y"][live].astype(np.int64)
    close = (np.abs(px[:, None] - px[None, :]) <= r) & (np.abs(py[:, None] - py[None, :]) <= r)
    return (int(close.sum()) - len(px)) // 2


# ------------------------------------------------------------------------------------------------------------------------ lists
def random_list(n, ncols, nrows, seed, max_age=4):
    """n tracked records spread over the frame (sub-pixel positions) and ages 0 .. max_age"""
    rs = np.random.RandomState(seed)
    out = records(rs.uniform(0, ncols, n).astype(np.float32), rs.uniform(0, nrows, n).astype(np.float32), 0, np.arange(n) * 7 + 1)
    out["x"] = np.minimum(out["x"], np.nextafter(np.float32(ncols), np.float32(0)))
    out["y"] = np.minimum(out["y"], np.nextafter(np.float32(nrows), np.float32(0)))
    return out, crowd_records(rs.randint(0, max_age + 1, n))


def non_candidate_kinds(out, ncols, nrows, start=0, step=1):
    """turns records start, start + step, ... of `out` into one non-candidate of every kind each, in place: the lost statuses -1 .. -9,
    a val > 0, NaN, +-inf, x just below 0, x = ncols, y likewise -- and, between them, candidates at the edges of the test: x = -0.0 and
    x just below ncols as f32.  -> (the non-candidates' record numbers, the edge candidates')"""
    below0 = np.nextafter(np.float32(0), np.float32(-1))
    kinds = [("val", v) for v in range(-1, -10, -1)] + [("val", 5), ("x", np.nan), ("y", np.nan), ("x", np.inf), ("x", -np.inf),
                                                         ("y", np.inf), ("y", -np.inf), ("x", below0), ("y", below0),
                                                         ("x", np.float32(ncols)), ("y", np.float32(nrows)), ("x", np.float32(-1.0))]
    edges = [("x", np.float32(-0.0)), ("y", np.float32(-0.0)), ("x", np.nextafter(np.float32(ncols), np.float32(0))),
             ("y", np.nextafter(np.float32(nrows), np.float32(0)))]
    where = [start + k * step for k in range(len(kinds) + len(edges))]
    assert where[-1] < len(out)
    for i, (field, value) in zip(where, kinds + edges):
        out[field][i] = value
    non, edge = where[:len(kinds)], where[len(kinds):]
    cand = candidate_mask(out, ncols, nrows)
    assert not cand[non].any() and cand[edge].all()
    return non, edge


def chain(count, r, x0=3.0, y0=5.0, dx=1, dy=0, reverse=False):
    """`count` candidates spaced r apart along (dx, dy) with ages falling along the line (rising, `reverse`): each is covered by its
    older neighbour alone, so the walk alternates kept / crowded and the rounds are as many as the candidates"""
    k = np.arange(count)
    out = records((x0 + k * r * dx + 0.25).astype(np.float32), (y0 + k * r * dy + 0.5).astype(np.float32), 0, k)
    age = (k if reverse else count - 1 - k) + 1
    return out, crowd_records(age)


def border_pairs(ncols, nrows, r, side):
    """pairs exactly r and r + 1 apart across a border of the device's cells (squares of `side` pixels), in x, in y and diagonally, each
    pair far from the others; and candidates at (0, 0) and (ncols - 1, nrows - 1)"""
    pts = []
    b = side                                                 # a cell border: pixels b - 1 | b
    slots = [(b * (2 * k + 1), b * 3) for k in range(6)]     # group k around the corner of four cells at (bx, by)
    for k, gap in enumerate((r, r + 1)):
        lo = gap // 2 + 1
        bx, by = slots[3 * k]
        pts += [(bx - lo, by + 5), (bx - lo + gap, by + 5)]                          # across a border in x
        bx, by = slots[3 * k + 1]
        pts += [(bx + 5, by - lo), (bx + 5, by - lo + gap)]                          # in y
        bx, by = slots[3 * k + 2]
        pts += [(bx - lo, by - lo), (bx - lo + gap, by - lo + gap)]                  # diagonally
    pts += [(0, 0), (ncols - 1, nrows - 1)]
    pts = np.asarray(pts, np.float32)
    assert (pts[:, 0] < ncols).all() and (pts[:, 1] < nrows).all() and (pts >= 0).all()
    return records(pts[:, 0] + np.float32(0.5), pts[:, 1] + np.float32(0.25), 0, np.arange(len(pts))), None


# ------------------------------------------------------------------------------------------------------------------------ the clip
ZOOM = 0.96                    # per frame, about the frame centre: 12 frames bring features selected 10 px apart to 6.4 px


def zoom_out_clip(count=12, width=320, height=240, seed=31):
    """frames of a camera that backs away: frame k is frame 0's texture scaled by ZOOM ** k about the centre (periodic texture)"""
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(width, height, seed)
    frames = []
    for k in range(count):
        f = synth.warp_frame(base, np.eye(2) * ZOOM ** k)
        f.setflags(write=False)
        frames.append(f)
    return frames


def zoom_out_geometry(count, width, height, spacing, mindist):
    """the clip's geometry with nothing tracked: a lattice of points `spacing` apart scaled by ZOOM per frame -> the live pairs within
    mindist - 1 after every frame"""
    ys, xs = np.mgrid[spacing // 2:height:spacing, spacing // 2:width:spacing]
    x, y = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    pairs = []
    for k in range(count):
        s = ZOOM ** k
        fl = records((cx + (x - cx) * s).astype(np.float32), (cy + (y - cy) * s).astype(np.float32))
        pairs.append(live_pairs_within(fl, mindist - 1, width, height))
    return pairs
