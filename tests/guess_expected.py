"""The motion-prior rule (include/klt_gpu.h, klt_track_guess_async) composed from the CPU oracle's per-level step: the loop of
ko_track_features (oracle/klt_oracle.c) in Python over ko_track_feature on the level slices of ko.Pyramids, with the one change the rule
makes -- where the search of a feature starts.  Also the constant-velocity predictor in numpy float32, the forward-backward composition
with a prior, and the large-shift pairs the tests run on."""
import ctypes as C

import numpy as np

from fb_expected import fb_expected
from pyfeaturetrack_amd import synth

KLT_TRACKED, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_OOB, KLT_LARGE_RESIDUE = 0, -2, -3, -4, -5

FEAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("val", np.int32), ("aux", np.int32)])


def guess_counts(fin, guess):
    """which features start from their guess: live, guess.val >= 0, both coordinates finite"""
    if guess is None:
        return np.zeros(len(fin), bool)
    return (fin["val"] >= 0) & (guess["val"] >= 0) & np.isfinite(guess["x"]) & np.isfinite(guess["y"])


def guess_records(positions, valid=None):
    """(n, 2) positions -> guess records (val 0; -1 where `valid` is false)"""
    g = np.zeros(len(positions), FEAT_DTYPE)
    g["x"], g["y"] = positions[:, 0], positions[:, 1]
    if valid is not None:
        g["val"] = np.where(valid, 0, -1)
    return g


def guess_compose(ko, p, pyr1, pyr2, fin, guess, want_iters=False):
    """G(1, 2, in, guess): the records (x, y, val and the aux word the kernels write: 4 bits per visited level, iterations + 1 saturating at
    15) of `fin` tracked from pyr1 into pyr2 with every feature's search started at its guess, if that counts, else at its own position."""
    lib = ko.lib()
    L, ss = int(p.nPyramidLevels), float(p.subsampling)
    ncols, nrows = pyr1.ncols, pyr1.nrows
    counts = guess_counts(fin, guess)
    planes = [[pyr.level(which, r) for which in ("img", "gx", "gy")] for pyr in (pyr1, pyr2) for r in range(L)]
    ptr = [[a.ctypes.data_as(C.c_void_p) for a in lv] for lv in planes]
    out = fin.copy()
    iters = np.full((len(fin), L), -1, np.int32)
    for f in range(len(fin)):
        if fin["val"][f] < 0:
            continue
        xloc, yloc = float(fin["x"][f]), float(fin["y"][f])
        xout, yout = (float(guess["x"][f]), float(guess["y"][f])) if counts[f] else (xloc, yloc)
        for _ in range(L):
            xloc /= ss
            yloc /= ss
            xout /= ss
            yout /= ss
        val, aux = KLT_TRACKED, 0
        for r in range(L - 1, -1, -1):
            xloc *= ss
            yloc *= ss
            xout *= ss
            yout *= ss
            px, py, it = C.c_double(xout), C.c_double(yout), C.c_int(0)
            nr_, nc_ = planes[r][0].shape
            val = lib.ko_track_feature(C.c_double(xloc), C.c_double(yloc), C.byref(px), C.byref(py), *ptr[r], *ptr[L + r],
                                       C.c_int(nc_), C.c_int(nr_), C.byref(p), C.byref(it))
            xout, yout = px.value, py.value
            iters[f, r] = it.value
            aux |= (it.value + 1 if it.value < 14 else 15) << (4 * r)
            if val in (KLT_SMALL_DET, KLT_OOB):
                break
        oob = (val == KLT_OOB or xout < p.borderx or xout > ncols - 1 - p.borderx
               or yout < p.bordery or yout > nrows - 1 - p.bordery)
        if oob:
            out[f] = (-1.0, -1.0, KLT_OOB, aux)
        elif val in (KLT_SMALL_DET, KLT_LARGE_RESIDUE, KLT_MAX_ITERATIONS):
            out[f] = (-1.0, -1.0, val, aux)
        else:
            out[f] = (xout, yout, KLT_TRACKED, aux)
    return (out, iters) if want_iters else out


def predict_cv(prev, cur):
    """klt_predict_cv_async in numpy float32: cur + (cur - prev) for a slot tracked (val == KLT_TRACKED) from a live one, else no guess"""
    g = np.zeros(len(cur), FEAT_DTYPE)
    g["x"], g["y"], g["val"] = -1.0, -1.0, -1
    ok = (cur["val"] == KLT_TRACKED) & (prev["val"] >= 0)
    for k in ("x", "y"):
        c, q = cur[k].astype(np.float32), prev[k].astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            g[k][ok] = (c + (c - q).astype(np.float32)).astype(np.float32)[ok]
    g["val"][ok] = 0
    return g


def fb_guess_compose(ko, p, pyr1, pyr2, fin, guess, max_error):
    """(out, fwd, back): fwd = G(1, 2, in, guess), back = T(2, 1, fwd) with the plain oracle tracker, then the forward-backward rule.
    (aux words: fwd's and back's are composed here as well, the plain way back through guess_compose without a guess.)"""
    fwd = guess_compose(ko, p, pyr1, pyr2, fin, guess)
    back = guess_compose(ko, p, pyr2, pyr1, fwd, None)
    return fb_expected(fin, fwd, back, max_error), fwd, back


# (name, width, height, window, levels, subsampling, shift of frame 2, features): frame 2 is the texture of seed 21 moved by `shift`, far
# outside what the pyramid's search range reaches from the feature's own position
LARGE_SHIFT_CASES = [
    ("320x240_w7", 320, 240, 7, 2, 4, (41.3, -27.6), 150),
    ("251x187_w7", 251, 187, 7, 2, 4, (60.3, 35.4), 149),
    ("320x240_w15", 320, 240, 15, 3, 2, (70.3, -40.6), 150),
    ("320x240_w9", 320, 240, 9, 2, 2, (41.3, -27.6), 150),
]


def large_shift_pair(width, height, shift, seed=21):
    base = synth.synth_base(width, height, seed)
    return synth.shift_frame(base, 0.0, 0.0), synth.shift_frame(base, shift[0], shift[1])


def noisy_truth(fin, shift, noise=2.0, seed=3):
    """(guess records, true positions): the true frame-2 position of every feature plus uniform noise in [-noise, noise] px"""
    truth = np.stack([fin["x"].astype(np.float64) + shift[0], fin["y"].astype(np.float64) + shift[1]], axis=1)
    jitter = np.random.RandomState(seed).uniform(-noise, noise, truth.shape)
    return guess_records((truth + jitter).astype(np.float32)), truth


def well_inside(truth, p, ncols, nrows, margin=2.0):
    """features whose true target lies more than `margin` px inside the border"""
    return ((truth[:, 0] > p.borderx + margin) & (truth[:, 0] < ncols - 1 - p.borderx - margin)
            & (truth[:, 1] > p.bordery + margin) & (truth[:, 1] < nrows - 1 - p.bordery - margin))
