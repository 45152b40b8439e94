"""The two integer rules of include/klt_gpu.h, "descriptors" (DESIGN.md section 9n), restated in numpy: the 256-bit descriptor of a feature
on an 8-bit frame and the brute-force Hamming match of two descriptor sets.  The device output equals what stands here byte for byte;
no tolerance appears anywhere.  Also the seeded trial functions the GPU tests run (as tests/equalize_expected.py has them)."""
import numpy as np

FEAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("val", np.int32), ("aux", np.int32)])
DESC_DTYPE = np.dtype([("bits", np.uint32, (8,)), ("val", np.int32), ("orientation", np.int32), ("cx", np.int32), ("cy", np.int32)])
MATCH_DTYPE = np.dtype([("train", np.int32), ("distance", np.int32), ("second", np.int32), ("val", np.int32)])
assert DESC_DTYPE.itemsize == 48 and MATCH_DTYPE.itemsize == 16

UPRIGHT, STEERED = 1, 2
NTESTS, REACH, BOX, DISC = 256, 13, 2, 15          # tests; largest test coordinate; half side of the box; radius of the orientation disc
NO_SECOND = 257
NOT_DESCRIBED, MATCHED, NO_CANDIDATE, TOO_FAR, AMBIGUOUS, NOT_MUTUAL = 0, 1, 2, 3, 4, 5       # klt_match.val

# C[k] = round(16384 cos(2 pi k / 32)), S[k] = C[(k + 24) % 32]: literal integers, as in the header
C = (16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
     -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069)
S = tuple(C[(k + 24) % 32] for k in range(32))


def pattern():
    """the 256 tests (ax, ay, bx, by) as an int32 [256][4] array, and the number of draws consumed"""
    state = [0x9E3779B9, 0]

    def draw():
        state[0] = (state[0] * 1664525 + 1013904223) & 0xFFFFFFFF
        state[1] += 1
        return ((state[0] >> 16) % 27) - 13
    tests, seen = [], set()
    while len(tests) < NTESTS:
        ax, ay, bx, by = draw(), draw(), draw(), draw()
        if ax * ax + ay * ay > 169 or bx * bx + by * by > 169 or (ax, ay) == (bx, by):
            continue
        if (ax, ay, bx, by) in seen or (bx, by, ax, ay) in seen:
            continue
        seen.add((ax, ay, bx, by))
        tests.append((ax, ay, bx, by))
    return np.array(tests, dtype=np.int32), state[1]


PATTERN, PATTERN_DRAWS = pattern()


def steered_pattern(k):
    """the pattern's points rotated by orientation bin k (k == 0: the pattern itself); the shift is a floor"""
    if k == 0:
        return PATTERN.astype(np.int64)
    p = PATTERN.astype(np.int64).reshape(-1, 2)
    xs = (p[:, 0] * C[k] - p[:, 1] * S[k] + 8192) >> 14
    ys = (p[:, 0] * S[k] + p[:, 1] * C[k] + 8192) >> 14
    return np.stack([xs, ys], axis=1).reshape(-1, 4)


_DV, _DU = np.mgrid[-DISC:DISC + 1, -DISC:DISC + 1]
_IN_DISC = (_DU * _DU + _DV * _DV) <= DISC * DISC


def centre(x, y, val, ncols, nrows):
    """(describable, cx, cy) of one feature record"""
    x, y = float(np.float32(x)), float(np.float32(y))
    if val < 0 or not np.isfinite(x) or not np.isfinite(y):
        return False, 0, 0
    cx, cy = np.floor(x + 0.5), np.floor(y + 0.5)
    if not (0 <= cx < ncols and 0 <= cy < nrows):
        return False, 0, 0
    return True, int(cx), int(cy)


def describe_one(frame, cx, cy, mode):
    """(bits as 8 uint32, orientation) of a describable centre"""
    nrows, ncols = frame.shape
    half = REACH + BOX                                   # 15: the patch is 31 x 31
    ys = np.clip(np.arange(cy - half, cy + half + 1), 0, nrows - 1)
    xs = np.clip(np.arange(cx - half, cx + half + 1), 0, ncols - 1)
    patch = frame[np.ix_(ys, xs)].astype(np.int64)       # patch[v + 15][u + 15] = P(u, v)
    k = 0
    if mode == STEERED:
        m10 = int((_DU * patch)[_IN_DISC].sum())
        m01 = int((_DV * patch)[_IN_DISC].sum())
        scores = [m10 * C[j] + m01 * S[j] for j in range(32)]
        k = scores.index(max(scores))                    # the smallest index among the maxima
    sat = np.zeros((32, 32), np.int64)
    sat[1:, 1:] = patch.cumsum(0).cumsum(1)
    side = 2 * BOX + 1
    box = sat[side:, side:] - sat[:-side, side:] - sat[side:, :-side] + sat[:-side, :-side]      # box[v + 13][u + 13] = B(u, v)
    t = steered_pattern(k)
    a = box[t[:, 1] + REACH, t[:, 0] + REACH]
    b = box[t[:, 3] + REACH, t[:, 2] + REACH]
    bit = (a < b).astype(np.uint8)
    words = np.packbits(bit, bitorder="little").view("<u4")
    return words, k


def describe(frame, feats, mode=UPRIGHT):
    """rule 1: DESC_DTYPE records of `feats` (FEAT_DTYPE, or anything with x, y, val fields) on the uint8 frame [nrows][ncols]"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 2 and mode in (UPRIGHT, STEERED)
    nrows, ncols = frame.shape
    out = np.zeros(len(feats), DESC_DTYPE)
    for i in range(len(feats)):
        ok, cx, cy = centre(feats["x"][i], feats["y"][i], int(feats["val"][i]), ncols, nrows)
        if not ok:
            continue
        words, k = describe_one(frame, cx, cy, mode)
        out[i] = (words, 1, k, cx, cy)
    return out


def features(xs, ys, vals=None):
    f = np.zeros(len(xs), FEAT_DTYPE)
    f["x"], f["y"] = xs, ys
    f["val"] = 0 if vals is None else vals
    return f


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distances(q, t):
    """[nq][nt] Hamming distances of the records' bits"""
    qb = np.ascontiguousarray(q["bits"]).view(np.uint8).reshape(len(q), 32)
    tb = np.ascontiguousarray(t["bits"]).view(np.uint8).reshape(len(t), 32)
    d = np.zeros((len(q), len(t)), np.int32)
    for w in range(32):
        d += _POP8[qb[:, w, None] ^ tb[None, :, w]]
    return d


def params_ok(max_distance, ratio_num, ratio_den, cross_check, radius):
    return (0 <= max_distance <= 256 and (ratio_num == 0 or 0 < ratio_num <= ratio_den <= 65535) and cross_check in (0, 1)
            and radius >= 0)


def _nearest(d, cand):
    """per row: (best column -- ties to the lowest --, its distance, the second distance), -1 / 257 / 257 where there is none"""
    n = d.shape[0]
    big = np.where(cand, d, NO_SECOND).astype(np.int32)
    if d.shape[1] == 0:
        return np.full(n, -1, np.int32), np.full(n, NO_SECOND, np.int32), np.full(n, NO_SECOND, np.int32)
    best = big.argmin(axis=1).astype(np.int32)           # (argmin: the first of equal minima)
    dist = big[np.arange(n), best]
    rest = big.copy()
    rest[np.arange(n), best] = NO_SECOND
    second = rest.min(axis=1)
    best[dist == NO_SECOND] = -1
    return best, dist, second


def match(q, t, max_distance=64, ratio_num=4, ratio_den=5, cross_check=1, radius=0):
    """rule 2: MATCH_DTYPE records, one per query"""
    assert params_ok(max_distance, ratio_num, ratio_den, cross_check, radius)
    nq, nt = len(q), len(t)
    out = np.zeros(nq, MATCH_DTYPE)
    d = distances(q, t)
    cand = (q["val"][:, None] == 1) & (t["val"][None, :] == 1)
    if radius > 0:
        cand &= np.abs(q["cx"][:, None].astype(np.int64) - t["cx"][None, :]) <= radius
        cand &= np.abs(q["cy"][:, None].astype(np.int64) - t["cy"][None, :]) <= radius
    best, dist, second = _nearest(d, cand)
    back = _nearest(d.T, cand.T)[0]                      # each train record's best query
    for i in range(nq):
        if q["val"][i] != 1:
            out[i] = (-1, 0, 0, NOT_DESCRIBED)
        elif best[i] < 0:
            out[i] = (-1, NO_SECOND, NO_SECOND, NO_CANDIDATE)
        else:
            di, si = int(dist[i]), int(second[i])
            if di > max_distance:
                val = TOO_FAR
            elif ratio_num and not di * ratio_den < si * ratio_num:
                val = AMBIGUOUS
            elif cross_check and back[best[i]] != i:
                val = NOT_MUTUAL
            else:
                val = MATCHED
            out[i] = (best[i], di, si, val)
    return out


def splits_for(nq, nt):
    """how many ranges the train set of a match is cut into (describe_rule.h, match_splits): enough that the launch has about 512
    workgroups, no range shorter than one tile of 256 records, at most 64"""
    if nq <= 0 or nt <= 0:
        return 1
    blocks = (nq + 63) // 64
    want = (512 + blocks - 1) // blocks
    tiles = (nt + 255) // 256
    return max(1, min(want, tiles, 64))


SPLIT_SHAPES = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 255), (1, 256), (1, 257), (3, 1000), (64, 1000), (65, 1000), (257, 1000), (300, 5000),
                (5000, 5000), (20000, 20000), (32768, 256), (32769, 512), (1, 16384), (1, 16385), (1, 1 << 20), (100000, 100000)]


# ---- the golden pair: the rule's discrimination, counted the same way on the host and on the device
def golden_pair(golden_dir, read_pgm):
    """(img0, img1, the 100 features selected on img0, the same features tracked into img1)"""
    import os
    g = np.load(os.path.join(golden_dir, "cfg1.npz"))
    return (read_pgm(os.path.join(golden_dir, "img0.pgm")), read_pgm(os.path.join(golden_dir, "img1.pgm")),
            features(g["sel100_x"], g["sel100_y"], g["sel100_val"]), features(g["trk100_r10_x"], g["trk100_r10_y"], g["trk100_r10_val"]))


def golden_counts(describe, match, golden_pair):
    """{(mode, radius): (matched, wrong, the lost tracks' queries by val code 3, 4, 5)} with `describe(frame, feats, mode)` and
    `match(q, t, radius)` under the default parameters -- shared with the device test"""
    img0, img1, f0, f1 = golden_pair
    lost = f1["val"] < 0
    out = {}
    for mode in (UPRIGHT, STEERED):
        q, t = describe(img0, f0, mode), describe(img1, f1, mode)
        for radius in (0, 20):
            m = match(q, t, radius)
            ok = m["val"] == MATCHED
            out[mode, radius] = (int(ok.sum()), int((m["train"][ok] != np.flatnonzero(ok)).sum()),
                                 tuple(int((m["val"][lost] == code).sum()) for code in (3, 4, 5)))
    return out


GOLDEN_COUNTS = {(UPRIGHT, 0): (89, 0, (5, 5, 1)), (STEERED, 0): (81, 0, None), (UPRIGHT, 20): (89, 0, None),
                 (STEERED, 20): (85, 0, None)}


def check_golden_counts(counts):
    for key, (matched, wrong, lost) in GOLDEN_COUNTS.items():
        assert counts[key][:2] == (matched, wrong), (key, counts[key])
        if lost is not None:
            assert counts[key][2] == lost, (key, counts[key])


# ---- seeded trials of the GPU tests
def random_frame(rng, ncols, nrows, kind):
    if kind == "constant":
        return np.full((nrows, ncols), int(rng.integers(0, 256)), np.uint8)
    if kind == "two":
        lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
        return np.where(rng.random((nrows, ncols)) < 0.5, lo, hi).astype(np.uint8)
    return rng.integers(0, 256, (nrows, ncols), dtype=np.uint8)


def random_features(rng, n, ncols, nrows):
    """positions over and a little beyond the frame, some on half-pixel positions, some lost, some not finite"""
    f = np.zeros(n, FEAT_DTYPE)
    f["x"] = rng.uniform(-2.0, ncols + 1.0, n).astype(np.float32)
    f["y"] = rng.uniform(-2.0, nrows + 1.0, n).astype(np.float32)
    half = rng.random(n) < 0.2
    f["x"][half] = np.floor(f["x"][half]) + np.float32(0.5)
    f["val"] = rng.integers(-3, 1000, n)
    f["val"][rng.random(n) < 0.7] = 0
    odd = rng.random(n) < 0.05
    f["x"][odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32), int(odd.sum()))
    f["aux"] = rng.integers(-5, 5, n)
    return f


def describe_draw(seed):
    """one seeded describe trial: (frame, feats, mode)"""
    rng = np.random.default_rng(9000 + seed)
    ncols, nrows = (int(v) for v in rng.integers(1, 90, 2))
    frame = random_frame(rng, ncols, nrows, ("random", "random", "two", "constant")[seed % 4])
    n = int(rng.choice([1, 3, 5, 63, 64, 65, 130]))
    return frame, random_features(rng, n, ncols, nrows), UPRIGHT + seed % 2


def random_bases(rng, centres):
    return rng.integers(0, 2 ** 32, (max(centres, 1), 8), dtype=np.uint64).astype(np.uint32)


def random_descriptors(rng, n, spread=12, centres=8, extent=200, base=None):
    """n records around a few random centres (`base`, or new ones) so that distances are small, ties and near-ties common; some
    undescribed"""
    if base is None:
        base = random_bases(rng, centres)
    out = np.zeros(n, DESC_DTYPE)
    if n == 0:
        return out
    out["bits"] = base[rng.integers(0, len(base), n)]
    for i in range(n):
        for b in rng.integers(0, 256, int(rng.integers(0, spread + 1))):
            out["bits"][i, b >> 5] ^= np.uint32(1 << (b & 31))
    out["val"] = (rng.random(n) < 0.85).astype(np.int32)
    out["orientation"] = rng.integers(0, 32, n)
    out["cx"] = rng.integers(0, extent, n)
    out["cy"] = rng.integers(0, extent, n)
    dead = out["val"] == 0
    out["bits"][dead] = 0
    out["orientation"][dead] = out["cx"][dead] = out["cy"][dead] = 0
    return out


def match_draw(seed):
    """one seeded match trial: (query, train, parameters)"""
    rng = np.random.default_rng(7000 + seed)
    nq = int(rng.choice([1, 2, 63, 64, 65, 130, 300]))
    nt = int(rng.choice([1, 2, 255, 256, 257, 700, 1500]))
    base = random_bases(rng, int(rng.integers(1, 9)))
    q = random_descriptors(rng, nq, base=base if seed % 3 else None)
    t = random_descriptors(rng, nt, base=base)
    if seed % 3 == 0 and nq and nt:                          # queries that are noisy copies of train records
        pick = rng.integers(0, nt, nq)
        q["bits"] = t["bits"][pick]
        q["cx"], q["cy"], q["val"] = t["cx"][pick], t["cy"][pick], t["val"][pick]
        for i in range(nq):
            for b in rng.integers(0, 256, int(rng.integers(0, 6))):
                q["bits"][i, b >> 5] ^= np.uint32(1 << (b & 31))
        q["bits"][q["val"] == 0] = 0
    den = int(rng.integers(1, 65536))
    params = dict(max_distance=int(rng.integers(0, 257)), ratio_num=int(rng.integers(0, den + 1)) if seed % 4 else 0, ratio_den=den,
                  cross_check=int(seed % 2), radius=int(rng.choice([0, 0, 1, 20, 60, 500])))
    return q, t, params
