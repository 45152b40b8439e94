"""The epipolar check (include/klt_gpu.h, "epipolar check") restated in numpy: float64 scalars and arrays, one
rounding per operation, python ints for `mix`, scalar python loops for `null9`.  `epipolar_check_expected` is what
klt_epipolar_check_async must leave behind, byte for byte, in `out` and in the model record.  Also here: klt_epipolar_matrix restated
and the seeded parallax scene of the tests."""
import struct

import numpy as np

from model_expected import FEAT_DTYPE, KLT_TRACKED, _sum64, candidate_mask, centred, mix, mulhi32, records

KLT_EPIPOLAR_OUTLIER = -8
EPIPOLAR_DTYPE = np.dtype([("f", np.float64, (9,)), ("valid", np.int32), ("n_candidates", np.int32), ("n_inliers", np.int32),
                           ("hypothesis", np.int32), ("hypothesis_inliers", np.int32), ("pad", np.int32)])
assert EPIPOLAR_DTYPE.itemsize == 96
DEFAULTS = dict(hypotheses=512, seed=0, min_inliers=16, max_error=1.0)
_M32 = 0xFFFFFFFF


def picks(seed, h, m):
    """the eight candidate numbers of hypothesis h among m candidates"""
    return tuple(mulhi32(mix((seed & _M32) ^ mix((8 * h + j) & _M32)), m) for j in range(8))


def scale_of(ncols, nrows):
    """s = 2^-k, k the smallest integer with 2 * (1 << k) >= max(ncols, nrows)"""
    k = 0
    while 2 * (1 << k) < max(ncols, nrows):
        k += 1
    return np.float64(2.0) ** -k


def _abs_bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0] & 0x7FFFFFFFFFFFFFFF


def _pow2(field):
    return np.float64(struct.unpack("<d", struct.pack("<Q", field << 52))[0])


def _traced(trace, event):
    if trace is not None:
        (trace if callable(trace) else trace.append)(event)


def null9(A, trace=None):
    """the null vector of an 8x9 matrix by the rule's division-free elimination with full pivoting, or None.  `trace` (a list or a
    callback; it changes nothing of the result) gets one dict per step k: the pivot's column is the ninth (`pc8`), another entry of the
    block holds the pivot's key (`tie`), rows / columns changed places (`row_swap`, `col_swap`), and `fail`: None, or why the step gave
    up -- "zero", "subnormal" or "nonfinite"."""
    A = np.array(A, np.float64)
    assert A.shape == (8, 9)
    perm = list(range(9))
    with np.errstate(all="ignore"):
        for k in range(8):
            best, br, bc, ties = -1, k, k, 0
            for i in range(k, 8):
                for j in range(k, 9):
                    b = _abs_bits(A[i, j])
                    if b > best:                    # (rows, then columns, in increasing order: the first of the largest)
                        best, br, bc, ties = b, i, j, 0
                    elif b == best:
                        ties += 1
            ef = best >> 52
            _traced(trace, dict(k=k, pc8=bc == 8, tie=ties > 0, row_swap=br != k, col_swap=bc != k,
                                fail=None if 0 < ef < 0x7FF else "nonfinite" if ef else "subnormal" if best else "zero"))
            if ef == 0 or ef == 0x7FF:
                return None
            A[[k, br], :] = A[[br, k], :]
            A[:, [k, bc]] = A[:, [bc, k]]
            perm[k], perm[bc] = perm[bc], perm[k]
            sc = _pow2(2045 - ef)
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


def rows_of(px, py, qx, qy):
    """the coefficients of q^T F p, F row-major: one row of nine per correspondence"""
    one = np.ones_like(px)
    return np.stack([qx * px, qx * py, qx, qy * px, qy * py, qy, px, py, one], axis=-1)


def working(fin, fout, cand, ncols, nrows):
    s = scale_of(ncols, nrows)
    return tuple(v * s for v in centred(fin, fout, cand, ncols, nrows))


def inliers(f, px, py, qx, qy, t2):
    a0 = (f[0] * px + f[1] * py) + f[2]
    a1 = (f[3] * px + f[4] * py) + f[5]
    a2 = (f[6] * px + f[7] * py) + f[8]
    b0 = (f[0] * qx + f[3] * qy) + f[6]
    b1 = (f[1] * qx + f[4] * qy) + f[7]
    r = (a0 * qx + a1 * qy) + a2
    den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
    return r * r <= t2 * den


def threshold2(max_error, ncols, nrows):
    ts = np.float64(np.float32(max_error)) * scale_of(ncols, nrows)
    return ts * ts


def hypothesis_of(px, py, qx, qy, seed, h):
    r = np.array(picks(seed, h, len(px)), np.int64)
    return null9(rows_of(px[r], py[r], qx[r], qy[r]))


def scores_expected(px, py, qx, qy, hypotheses, seed, t2):
    scores = np.full(hypotheses, -1, np.int64)
    with np.errstate(all="ignore"):
        for h in range(hypotheses):
            f = hypothesis_of(px, py, qx, qy, seed, h)
            if f is not None:
                scores[h] = int(inliers(f, px, py, qx, qy, t2).sum())
    return scores


def normal_matrix(px, py, qx, qy, inl):
    """M = SUM row^T row over the inliers: 45 sums in the partial scheme of the motion-model rule, mirrored"""
    rows = rows_of(px, py, qx, qy)
    M = np.zeros((9, 9), np.float64)
    for i in range(9):
        for j in range(i, 9):
            M[i, j] = M[j, i] = _sum64(rows[:, i] * rows[:, j], inl)
    return M


def free_index(f):
    """g: the index of the largest |f_i|, ties to the smallest"""
    g = 0
    for i in range(1, 9):
        if abs(f[i]) > abs(f[g]):
            g = i
    return g


def refit(px, py, qx, qy, inl, f):
    M = normal_matrix(px, py, qx, qy, inl)
    return null9(np.delete(M, free_index(f), axis=0))


def _record(ncols, nrows, m, f=None, valid=0, n_inliers=0, hyp=-1, hyp_inliers=0):
    rec = np.zeros((), EPIPOLAR_DTYPE)
    if f is not None:
        rec["f"] = f
    rec["valid"], rec["n_candidates"], rec["n_inliers"] = valid, m, n_inliers
    rec["hypothesis"], rec["hypothesis_inliers"] = hyp, hyp_inliers
    rec["pad"] = np.array(ncols | (nrows << 16), np.uint32).view(np.int32)
    return rec


def epipolar_check_expected(fin, fout, ncols, nrows, hypotheses=512, seed=0, min_inliers=16, max_error=1.0):
    """(out, model record): what the check leaves in `out` and in the model buffer; a pure function of its input"""
    fin = np.ascontiguousarray(fin, FEAT_DTYPE)
    out = np.ascontiguousarray(fout, FEAT_DTYPE).copy()
    cand = candidate_mask(fin, out, ncols, nrows)
    m = int(cand.sum())
    if m < min_inliers:
        return out, _record(ncols, nrows, m)
    px, py, qx, qy = working(fin, out, cand, ncols, nrows)
    t2 = threshold2(max_error, ncols, nrows)
    scores = scores_expected(px, py, qx, qy, hypotheses, seed, t2)
    best = int(np.argmax(scores))                   # the first of the largest: ties go to the smallest h
    if scores[best] < min_inliers:
        return out, _record(ncols, nrows, m)
    with np.errstate(all="ignore"):
        hyp = hypothesis_of(px, py, qx, qy, seed, best)
        inl = inliers(hyp, px, py, qx, qy, t2)
        assert int(inl.sum()) == scores[best]
        fit = refit(px, py, qx, qy, inl, hyp)
        model, valid = (fit, 1) if fit is not None else (hyp, 2)
        final = inliers(model, px, py, qx, qy, t2)
    idx = np.flatnonzero(cand)[~final]
    out["x"][idx] = -1.0
    out["y"][idx] = -1.0
    out["val"][idx] = KLT_EPIPOLAR_OUTLIER
    return out, _record(ncols, nrows, m, model, valid, int(final.sum()), best, int(scores[best]))


def epipolar_matrix(rec):
    """klt_epipolar_matrix: T^T F T in uncentred pixels, scaled to unit Frobenius norm, or None for valid == 0"""
    if int(rec["valid"]) == 0:
        return None
    pad = int(np.array(rec["pad"], np.int32).view(np.uint32))
    ncols, nrows = pad & 0xFFFF, pad >> 16
    s = scale_of(ncols, nrows)
    cx, cy = np.float64(ncols // 2), np.float64(nrows // 2)
    f = np.asarray(rec["f"], np.float64)
    # G = T^T F T, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], written out entry by entry in the order of the C code
    u, v = -(s * cx), -(s * cy)
    r0 = (s * f[0], s * f[1], (f[0] * u + f[1] * v) + f[2])         # rows of F T
    r1 = (s * f[3], s * f[4], (f[3] * u + f[4] * v) + f[5])
    r2 = (s * f[6], s * f[7], (f[6] * u + f[7] * v) + f[8])
    g = [s * r0[0], s * r0[1], s * r0[2],
         s * r1[0], s * r1[1], s * r1[2],
         (u * r0[0] + v * r1[0]) + r2[0], (u * r0[1] + v * r1[1]) + r2[1], (u * r0[2] + v * r1[2]) + r2[2]]
    g = np.array(g, np.float64)
    nrm = np.float64(0.0)
    for e in g:
        nrm = nrm + e * e
    nrm = np.sqrt(nrm)
    if not (nrm > 0) or not np.isfinite(nrm):
        return None
    return g / nrm


# ---------------------------------------------------------------------------------------------------------------- the parallax scene
SCENES = {"oblique": ((0.3, 0.02, 0.05), 60), "sideways": ((0.3, 0.0, 0.0), 60), "forward": ((0.0, 0.0, 0.5), 150)}


def parallax_lists(name, seed, ncols=1920, nrows=1080, focal=1000.0, npoints=600, noise=0.1):
    """600 points in [-8, 8] x [-4.5, 4.5] x [4, 30] seen by a camera of focal length 1000 px before and after a step (rotation 0.01 rad
    about y, 0.005 about x, the scene's translation), 0.1 px Gaussian noise on frame 2, the first tracks displaced by
    uniform(-15, 15) + 3 * sign per axis, points off the frame dropped.  Returns (in, out, moved mask)."""
    t, nmoved = SCENES[name]
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-8, 8, npoints), rs.uniform(-4.5, 4.5, npoints), rs.uniform(4, 30, npoints)])
    ay, ax = 0.01, 0.005
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    X2 = Rx @ Ry @ X - np.array(t)[:, None]
    c = np.array([ncols / 2.0, nrows / 2.0])
    p = focal * X[:2] / X[2] + c[:, None]
    q = focal * X2[:2] / X2[2] + c[:, None]
    q = q + rs.normal(0.0, noise, q.shape)
    moved = np.zeros(npoints, bool)
    moved[:nmoved] = True
    d = rs.uniform(-15, 15, (2, nmoved))
    q[:, :nmoved] += d + 3 * np.sign(d)
    keep = (p[0] >= 0) & (p[0] < ncols - 1) & (p[1] >= 0) & (p[1] < nrows - 1) & (q[0] >= 0) & (q[0] < ncols - 1) & (q[1] >= 0) & (q[1] < nrows - 1)
    fin = records(p[0][keep], p[1][keep], rs.randint(0, 1000, int(keep.sum())), 0)
    fout = records(q[0][keep], q[1][keep], KLT_TRACKED, rs.randint(-5, 5, int(keep.sum())))
    return fin, fout, moved[keep]


def translation_lists(n, ncols, nrows, seed, shift=(3, -2)):
    """exact integer positions under a pure integer translation: every eight rows span at most six dimensions"""
    rs = np.random.RandomState(seed)
    x = rs.randint(16, ncols - 16, n)
    y = rs.randint(16, nrows - 16, n)
    return records(x, y, 0, 0), records(x + shift[0], y + shift[1], KLT_TRACKED, rs.randint(-5, 5, n))


def parallax_n(n, ncols, nrows, seed, moved_part=0.1, t=(0.3, 0.02, 0.05), noise=0.1):
    """exactly n records of the parallax scene's kind on a frame of any size (focal length ncols / 1.92, as 1000 px is for 1920 columns);
    the first moved_part of them displaced.  Returns (in, out, moved mask)."""
    rs = np.random.RandomState(seed)
    focal = ncols / 1.92
    tot = 3 * n + 64
    X = np.stack([rs.uniform(-8, 8, tot), rs.uniform(-8.0 * nrows / ncols, 8.0 * nrows / ncols, tot), rs.uniform(4, 30, tot)])
    ay, ax = 0.01, 0.005
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    X2 = Rx @ Ry @ X - np.array(t)[:, None]
    c = np.array([ncols / 2.0, nrows / 2.0])
    p = focal * X[:2] / X[2] + c[:, None]
    q = focal * X2[:2] / X2[2] + c[:, None] + rs.normal(0.0, noise, (2, tot))
    d = rs.uniform(-15, 15, (2, tot))
    d = d + 3 * np.sign(d)
    keep = np.ones(tot, bool)
    for v, lim in ((p[0], ncols), (p[1], nrows), (q[0], ncols), (q[1], nrows), (q[0] + d[0], ncols), (q[1] + d[1], nrows)):
        keep &= (v >= 0) & (v < lim - 1)
    idx = np.flatnonzero(keep)[:n]
    assert len(idx) == n
    p, q, d = p[:, idx], q[:, idx], d[:, idx]
    moved = np.zeros(n, bool)
    moved[:int(n * moved_part)] = True
    q[:, moved] += d[:, moved]
    return records(p[0], p[1], rs.randint(0, 1000, n), 0), records(q[0], q[1], KLT_TRACKED, rs.randint(-5, 5, n)), moved


# ---------------------------------------------------------------------------------------------------------------- frames with parallax
LAYER_STEP = {"far": (3.0, 0.0), "near": (8.0, 0.0), "mover": (0.0, 5.0)}      # px per frame: a sideways camera step, and a block on its own
LAYER_NEAR_ROWS = (160, 240)
LAYER_MOVER = (40, 110, 110, 200)      # y0, y1, x0, x1


def layered_clip(count=6, width=320, height=240):
    """frames of a camera that steps sideways past two depths: the far texture moves 3 px per frame, the near one (the lowest rows) 8 px,
    both along the rows -- so the epipolar lines are the rows and F is unique --, and a block of a third texture moves 5 px per frame
    DOWN the columns, off every epipolar line by five times the default threshold"""
    from pyfeaturetrack_amd import synth
    far, near, mover = (synth.synth_base(width, height, s) for s in (21, 23, 22))
    y0, y1, x0, x1 = LAYER_MOVER
    frames = []
    for k in range(count):
        f = synth.shift_frame(far, LAYER_STEP["far"][0] * k, LAYER_STEP["far"][1] * k)
        n = synth.shift_frame(near, LAYER_STEP["near"][0] * k, LAYER_STEP["near"][1] * k)
        f[LAYER_NEAR_ROWS[0]:LAYER_NEAR_ROWS[1]] = n[LAYER_NEAR_ROWS[0]:LAYER_NEAR_ROWS[1]]
        f[y0:y1, x0:x1] = synth.shift_frame(mover, LAYER_STEP["mover"][0] * k, LAYER_STEP["mover"][1] * k)[y0:y1, x0:x1]
        f.setflags(write=False)
        frames.append(f)
    return frames


def inside_mover(fl, window, clear=3):
    """records whose window plus `clear` px lies wholly inside the moving block"""
    y0, y1, x0, x1 = LAYER_MOVER
    r = window // 2 + clear
    return (fl["x"] - r >= x0) & (fl["x"] + r <= x1 - 1) & (fl["y"] - r >= y0) & (fl["y"] + r <= y1 - 1)
