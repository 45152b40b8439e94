"""The homography check (include/klt_gpu.h, "homography check") restated in numpy: float64 scalars and arrays, one
rounding per operation.  `null9`, the working coordinates, the threshold and the free index are the epipolar rule's, imported from
tests/epipolar_expected.py unchanged.  `homography_check_expected` is what klt_homography_check_async must leave behind, byte for byte, in
`out` and in the model record.  Also here: klt_homography_matrix restated, the seeded rotation / plane scenes and a clip whose background
moves by a homography."""
import numpy as np

from epipolar_expected import free_index, null9, scale_of, threshold2, working
from model_expected import FEAT_DTYPE, KLT_TRACKED, _sum64, candidate_mask, mix, mulhi32, records

KLT_HOMOGRAPHY_OUTLIER = -9
HOMOGRAPHY_DTYPE = np.dtype([("h", np.float64, (9,)), ("valid", np.int32), ("n_candidates", np.int32), ("n_inliers", np.int32),
                             ("hypothesis", np.int32), ("hypothesis_inliers", np.int32), ("pad", np.int32)])
assert HOMOGRAPHY_DTYPE.itemsize == 96
DEFAULTS = dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0)
_M32 = 0xFFFFFFFF


def picks(seed, h, m):
    """the four candidate numbers of hypothesis h among m candidates"""
    return tuple(mulhi32(mix((seed & _M32) ^ mix((4 * h + j) & _M32)), m) for j in range(4))


def rows_of(px, py, qx, qy):
    """step 3: the two rows of every correspondence, interleaved (rows 2j and 2j + 1 belong to correspondence j): shape (2 n, 9)"""
    n = len(px)
    one, zero = np.ones(n, np.float64), np.zeros(n, np.float64)
    even = np.stack([px, py, one, zero, zero, zero, -(qx * px), -(qx * py), -qx], axis=-1)
    odd = np.stack([zero, zero, zero, px, py, one, -(qy * px), -(qy * py), -qy], axis=-1)
    return np.stack([even, odd], axis=1).reshape(2 * n, 9)


def inliers(h, px, py, qx, qy, t2):
    u = (h[0] * px + h[1] * py) + h[2]
    v = (h[3] * px + h[4] * py) + h[5]
    w = (h[6] * px + h[7] * py) + h[8]
    rx = u - w * qx
    ry = v - w * qy
    return rx * rx + ry * ry <= t2 * (w * w)


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
    """M = [[A, 0, -Bx], [0, A, -By], [-Bx, -By, C]]: 24 sums in the partial scheme of the motion-model rule, mirrored"""
    e = (px, py, np.ones(len(px), np.float64))
    qq = qx * qx + qy * qy
    A, Bx, By, C = (np.zeros((3, 3), np.float64) for _ in range(4))
    for i in range(3):
        for j in range(i, 3):
            ee = e[i] * e[j]
            A[i, j] = A[j, i] = _sum64(ee, inl)
            Bx[i, j] = Bx[j, i] = _sum64(qx * ee, inl)
            By[i, j] = By[j, i] = _sum64(qy * ee, inl)
            C[i, j] = C[j, i] = _sum64(qq * ee, inl)
    M = np.zeros((9, 9), np.float64)                # (the structural zeros: +0.0)
    M[0:3, 0:3] = A
    M[3:6, 3:6] = A
    M[6:9, 6:9] = C
    M[0:3, 6:9] = M[6:9, 0:3] = -Bx
    M[3:6, 6:9] = M[6:9, 3:6] = -By
    return M


def refit(px, py, qx, qy, inl, h):
    M = normal_matrix(px, py, qx, qy, inl)
    return null9(np.delete(M, free_index(h), axis=0))


def _record(ncols, nrows, m, h=None, valid=0, n_inliers=0, hyp=-1, hyp_inliers=0):
    rec = np.zeros((), HOMOGRAPHY_DTYPE)
    if h is not None:
        rec["h"] = h
    rec["valid"], rec["n_candidates"], rec["n_inliers"] = valid, m, n_inliers
    rec["hypothesis"], rec["hypothesis_inliers"] = hyp, hyp_inliers
    rec["pad"] = np.array(ncols | (nrows << 16), np.uint32).view(np.int32)
    return rec


def homography_check_expected(fin, fout, ncols, nrows, hypotheses=256, seed=0, min_inliers=8, max_error=1.0):
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
    out["val"][idx] = KLT_HOMOGRAPHY_OUTLIER
    return out, _record(ncols, nrows, m, model, valid, int(final.sum()), best, int(scores[best]))


def homography_matrix(rec):
    """klt_homography_matrix: T^-1 h T in uncentred pixels, scaled to unit Frobenius norm, the third coordinate positive at the image
    centre; None for valid == 0"""
    if int(rec["valid"]) == 0:
        return None
    pad = int(np.array(rec["pad"], np.int32).view(np.uint32))
    ncols, nrows = pad & 0xFFFF, pad >> 16
    s = scale_of(ncols, nrows)
    r = np.float64(1.0) / s
    cx, cy = np.float64(ncols // 2), np.float64(nrows // 2)
    h = np.asarray(rec["h"], np.float64)
    # G = h T, then P = T^-1 G, entry by entry in the order of the C code
    u, v = -(s * cx), -(s * cy)
    G = [(s * h[3 * i], s * h[3 * i + 1], (h[3 * i] * u + h[3 * i + 1] * v) + h[3 * i + 2]) for i in range(3)]
    P = [r * G[0][j] + cx * G[2][j] for j in range(3)] + [r * G[1][j] + cy * G[2][j] for j in range(3)] + [G[2][j] for j in range(3)]
    P = np.array(P, np.float64)
    nrm = np.float64(0.0)
    for e in P:
        nrm = nrm + e * e
    nrm = np.sqrt(nrm)
    if not (nrm > 0) or not np.isfinite(nrm):
        return None
    if h[8] < 0:
        nrm = -nrm
    return P / nrm


def transfer_error(H, fin, fout):
    """|q - H p| in pixels for every record, H a 3x3 matrix in pixel coordinates"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    p = np.stack([fin["x"].astype(np.float64), fin["y"].astype(np.float64), np.ones(len(fin))])
    hp = H @ p
    return np.hypot(hp[0] / hp[2] - fout["x"], hp[1] / hp[2] - fout["y"])


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _rot(ax, ay, az):
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


NMOVED = 60


def scene(name, seed, ncols=1920, nrows=1080, focal=1000.0, npoints=600, noise=0.1):
    """The geometry of epipolar_expected.parallax_lists with a motion that IS a homography: 600 points seen by a camera of focal length
    1000 px before and after
      "rotation"  a pure rotation of 0.03 rad about y, 0.01 about x, 0.02 about z (points in [-8, 8] x [-4.5, 4.5] x [4, 30]), or
      "plane"     a step (0.3, 0.05, 0.4) plus a rotation of 0.01 rad about y and 0.005 about x, all points on z = 8 + 0.5 x + 0.3 y;
    0.1 px Gaussian noise on frame 2, the first 60 tracks displaced by uniform(-15, 15) + 3 * sign per axis, points off the frame
    dropped.  Returns (in, out, moved mask, H): H the true homography in pixels."""
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-8, 8, npoints), rs.uniform(-4.5, 4.5, npoints), rs.uniform(4, 30, npoints)])
    K = np.array([[focal, 0, ncols / 2.0], [0, focal, nrows / 2.0], [0, 0, 1.0]])
    if name == "rotation":
        R = _rot(0.01, 0.03, 0.02)
        X2 = R @ X
        H = K @ R @ np.linalg.inv(K)
    else:
        X[2] = 8 + 0.5 * X[0] + 0.3 * X[1]
        R, t = _rot(0.005, 0.01, 0.0), np.array([0.3, 0.05, 0.4])
        X2 = R @ X - t[:, None]
        nrm = np.array([-0.5, -0.3, 1.0])            # the plane: nrm . X = 8
        H = K @ (R - np.outer(t, nrm) / 8.0) @ np.linalg.inv(K)
    p = K @ X
    q = K @ X2
    p, q = p[:2] / p[2], q[:2] / q[2]
    q = q + rs.normal(0.0, noise, q.shape)
    moved = np.zeros(npoints, bool)
    moved[:NMOVED] = True
    d = rs.uniform(-15, 15, (2, NMOVED))
    q[:, :NMOVED] += d + 3 * np.sign(d)
    keep = (p[0] >= 0) & (p[0] < ncols - 1) & (p[1] >= 0) & (p[1] < nrows - 1) & (q[0] >= 0) & (q[0] < ncols - 1) & (q[1] >= 0) & (q[1] < nrows - 1)
    fin = records(p[0][keep], p[1][keep], rs.randint(0, 1000, int(keep.sum())), 0)
    fout = records(q[0][keep], q[1][keep], KLT_TRACKED, rs.randint(-5, 5, int(keep.sum())))
    return fin, fout, moved[keep], H


def rotation_n(n, ncols, nrows, seed, moved_part=0.1, noise=0.1):
    """exactly n records of the rotation scene's kind on a frame of any size (focal length ncols / 1.92); the first moved_part of them
    displaced.  Returns (in, out, moved mask)."""
    rs = np.random.RandomState(seed)
    focal = ncols / 1.92
    K = np.array([[focal, 0, ncols / 2.0], [0, focal, nrows / 2.0], [0, 0, 1.0]])
    H = K @ _rot(0.01, 0.03, 0.02) @ np.linalg.inv(K)
    tot = 3 * n + 64
    p = np.stack([rs.uniform(0, ncols - 1, tot), rs.uniform(0, nrows - 1, tot), np.ones(tot)])
    q = H @ p
    q = q[:2] / q[2] + rs.normal(0.0, noise, (2, tot))
    d = rs.uniform(-15, 15, (2, tot))
    d = d + 3 * np.sign(d)
    keep = np.ones(tot, bool)
    for v, lim in ((q[0], ncols), (q[1], nrows), (q[0] + d[0], ncols), (q[1] + d[1], nrows)):
        keep &= (v >= 0) & (v < lim - 1)
    idx = np.flatnonzero(keep)[:n]
    assert len(idx) == n
    p, q, d = p[:2, idx], q[:, idx], d[:, idx]
    moved = np.zeros(n, bool)
    moved[:int(n * moved_part)] = True
    q[:, moved] += d[:, moved]
    return records(p[0], p[1], rs.randint(0, 1000, n), 0), records(q[0], q[1], KLT_TRACKED, rs.randint(-5, 5, n)), moved


def collinear_lists(n, ncols, nrows, seed, noise=0.0):
    """n candidates on one line of frame 1 (up to the rounding of the float32 coordinates), moved by a translation: a family of
    homographies fits them.  `noise` px of Gaussian noise on frame 2 makes every four-point hypothesis ill-conditioned instead."""
    rs = np.random.RandomState(seed)
    t = np.sort(rs.uniform(0.1, 0.9, n))
    x, y = t * (ncols - 1), 0.2 * nrows + 0.5 * t * (nrows - 1)
    d = rs.normal(0.0, 1.0, (2, n)) * noise
    return records(x, y, 0, 0), records(x + 3 + d[0], y - 2 + d[1], KLT_TRACKED, rs.randint(-5, 5, n))


# ---------------------------------------------------------------------------------------------------------------- frames under a homography
CLIP_MOVER = (40, 110, 110, 200)       # y0, y1, x0, x1
CLIP_MOVER_STEP = (0.0, 5.0)           # px per frame: the block's texture moves down the columns on its own


def clip_homography(k, width=320, height=240):
    """frame 0 -> frame k of the background: a pan with perspective about the frame centre, the same step k times"""
    c = np.array([[1, 0, width / 2.0], [0, 1, height / 2.0], [0, 0, 1.0]])
    step = np.array([[1.0, 0.004, 2.0], [-0.004, 1.0, 1.0], [4e-5, 2e-5, 1.0]])
    return c @ np.linalg.matrix_power(step, k) @ np.linalg.inv(c)


def warped_clip(count=6, width=320, height=240):
    """frames of a camera that pans with perspective -- the background texture of frame k is frame 0's warped by clip_homography(k): up to
    6 px at the frame's corners per step, its perspective part a pixel --, and a block of another texture that moves 5 px per frame down
    the columns on its own, five times the default threshold off the background's homography and more"""
    from pyfeaturetrack_amd import synth
    back, mover = synth.synth_base(width, height, 21), synth.synth_base(width, height, 22)
    y0, y1, x0, x1 = CLIP_MOVER
    frames = []
    for k in range(count):
        f = synth.warp_homography(back, clip_homography(k, width, height))
        f[y0:y1, x0:x1] = synth.shift_frame(mover, CLIP_MOVER_STEP[0] * k, CLIP_MOVER_STEP[1] * k)[y0:y1, x0:x1]
        f.setflags(write=False)
        frames.append(f)
    return frames


def inside_mover(fl, window, clear=3):
    """records whose window plus `clear` px lies wholly inside the moving block"""
    y0, y1, x0, x1 = CLIP_MOVER
    r = window // 2 + clear
    return (fl["x"] - r >= x0) & (fl["x"] + r <= x1 - 1) & (fl["y"] - r >= y0) & (fl["y"] + r <= y1 - 1)
