"""The track-quality rule (include/klt_gpu.h, klt_track_quality_async) restated in numpy over the CPU oracle's sampler
(`ko.extract_patch`) and numpy's pairwise f32 sum (`ko.abs_sum_f32`), one feature at a time -- and the lists the tests of the rule run on.

Every FP64 operation is written on its own (numpy rounds each once, nothing is contracted); the eight sums are kept as 64 partials, term k
joining partial k mod 64 in increasing k, and folded by p[l] += p[l + m], l < m, for m = 32 .. 1."""
import numpy as np

KLT_TRACKED, KLT_NOT_FOUND, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_OOB, KLT_LARGE_RESIDUE, KLT_FB_INCONSISTENT = 0, -1, -2, -3, -4, -5, -6
LOSS_CODES = (KLT_NOT_FOUND, KLT_SMALL_DET, KLT_MAX_ITERATIONS, KLT_OOB, KLT_LARGE_RESIDUE, KLT_FB_INCONSISTENT)

FEAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("val", np.int32), ("aux", np.int32)])
QUALITY_DTYPE = np.dtype([("residue", np.float32), ("ncc", np.float32), ("min_eig", np.float32), ("val", np.int32)])
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ the rule
def _inside(v, limit):
    """0 <= v < limit; NaN and the infinities fail (asked before v is converted to int)"""
    v = float(v)
    return v >= 0.0 and v < limit


def _window_fits(x, y, hw, ncols, nrows):
    ix, iy = int(F32(x)), int(F32(y))                # C's (int): towards zero (x is inside the frame here)
    return ix - hw >= 0 and iy - hw >= 0 and ix + hw + 2 <= ncols and iy + hw + 2 <= nrows


def measured(fin, fout, w, ncols, nrows):
    hw = w // 2
    if not (fin["val"] >= 0 and fout["val"] == KLT_TRACKED):
        return False
    if not (_inside(fin["x"], ncols) and _inside(fin["y"], nrows) and _inside(fout["x"], ncols) and _inside(fout["y"], nrows)):
        return False
    return _window_fits(fin["x"], fin["y"], hw, ncols, nrows) and _window_fits(fout["x"], fout["y"], hw, ncols, nrows)


def fold64(terms):
    """the FP64 sum of `terms` (float64, in order k) in the rule's order"""
    p = np.zeros(64, F64)
    for k0 in range(0, len(terms), 64):              # increasing k: one add per partial and round
        chunk = terms[k0:k0 + 64]
        p[:len(chunk)] = p[:len(chunk)] + chunk
    m = 32
    while m >= 1:
        p[:m] = p[:m] + p[m:2 * m]
        m //= 2
    return p[0]


def quality_record(ko, img1, img2, gx2, gy2, fin, fout, w):
    """(residue, ncc, min_eig, val) of one feature: img1 = frame 1's level-0 image; img2, gx2, gy2 = frame 2's level-0 image and gradients"""
    nrows, ncols = img1.shape
    if not measured(fin, fout, w, ncols, nrows):
        return (F32(0), F32(0), F32(0), 0)
    n = w * w
    T = ko.extract_patch(img1, fin["x"], fin["y"], w, w).ravel()
    S = ko.extract_patch(img2, fout["x"], fout["y"], w, w).ravel()
    Sgx = ko.extract_patch(gx2, fout["x"], fout["y"], w, w).ravel()
    Sgy = ko.extract_patch(gy2, fout["x"], fout["y"], w, w).ravel()
    residue = ko.abs_sum_f32(T - S) / F32(n)                         # f32 differences, numpy's pairwise sum, one f32 division
    Td, Sd, Xd, Yd = T.astype(F64), S.astype(F64), Sgx.astype(F64), Sgy.astype(F64)
    st, ss = fold64(Td), fold64(Sd)
    stt, sss, sts = fold64(Td * Td), fold64(Sd * Sd), fold64(Td * Sd)  # exact products of two f32
    gxx, gxy, gyy = fold64(Xd * Xd), fold64(Xd * Yd), fold64(Yd * Yd)
    nd = F64(n)
    with np.errstate(all="ignore"):
        a = nd * stt - st * st
        b = nd * sss - ss * ss
        c = nd * sts - st * ss
        ncc = F32(0)
        if a > 0 and b > 0:
            v = c / np.sqrt(a * b)
            if v < -1.0:
                v = F64(-1.0)
            if v > 1.0:
                v = F64(1.0)
            ncc = F32(v)
        d = gxx - gyy
        e = ((gxx + gyy) - np.sqrt(d * d + F64(4.0) * (gxy * gxy))) / F64(2.0)
        min_eig = F32(e) if e > 0 else F32(0)
    return (F32(residue), ncc, min_eig, 1)


def quality_expected(ko, pyr1, pyr2, fin, fout, w):
    """the QUALITY_DTYPE records of two lists on level 0 of two oracle pyramids (ko.Pyramids)"""
    img1 = pyr1.level("img", 0)
    img2, gx2, gy2 = (pyr2.level(which, 0) for which in ("img", "gx", "gy"))
    out = np.zeros(len(fin), QUALITY_DTYPE)
    for i in range(len(fin)):
        out[i] = quality_record(ko, img1, img2, gx2, gy2, fin[i], fout[i], w)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def records(xs, ys, val=KLT_TRACKED):
    fl = np.zeros(len(xs), FEAT_DTYPE)
    fl["x"], fl["y"], fl["val"] = xs, ys, val
    return fl


def edge_positions(w, ncols, nrows):
    """[(x, y, fits)]: for each of the four edges the last position whose window is inside the frame and the first one outside it, with
    integer and with fractional coordinates (ix - hw >= 0 and ix + hw + 2 <= ncols decide, ix = (int)x)"""
    hw = w // 2
    cx, cy = ncols // 2 + 0.25, nrows // 2 + 0.5
    out = []
    for frac in (0.0, 0.75):
        out += [(hw + frac, cy, True), (hw - 1 + frac, cy, False),                           # left
                (ncols - hw - 2 + frac, cy, True), (ncols - hw - 1 + frac, cy, False),       # right
                (cx, hw + frac, True), (cx, hw - 1 + frac, False),                           # top
                (cx, nrows - hw - 2 + frac, True), (cx, nrows - hw - 1 + frac, False)]       # bottom
    return out


def unmeasured_kinds(fin, fout, w, ncols, nrows, start=0):
    """Copies of the two lists with records start, start + 1, ... overwritten by every kind the rule does not measure -- and, among the
    window-edge positions, the last ones it still does.  Returns (fin, fout, {index: expected to be measured or not})."""
    fin, fout = fin.copy(), fout.copy()
    cx, cy = F32(ncols // 2 + 0.5), F32(nrows // 2 + 0.25)
    want = {}
    i = start

    def put(rin, rout, is_measured):
        nonlocal i
        fin[i], fout[i] = rin, rout
        want[i] = is_measured
        i += 1

    ok_in, ok_out = (cx, cy, 1, 0), (cx, cy, KLT_TRACKED, 0)
    put((cx, cy, KLT_OOB, 0), ok_out, False)                                  # lost `in`
    put((-1.0, -1.0, KLT_NOT_FOUND, 0), ok_out, False)
    for code in LOSS_CODES:                                                   # every loss code in `out`
        put(ok_in, (-1.0, -1.0, code, 0), False)
        put(ok_in, (cx, cy, code, 0), False)
    put(ok_in, (cx, cy, 1, 0), False)                                         # out.val > 0: refilled by a replacement pass
    put(ok_in, (cx, cy, 4711, 0), False)
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30, -0.5, None, float(max(ncols, nrows))):
        bad_x, bad_y = (float(ncols), float(nrows)) if bad is None else (bad, bad)       # None: the first coordinate off the frame, per axis
        put((bad_x, cy, 1, 0), ok_out, False)
        put((cx, bad_y, 1, 0), ok_out, False)
        put(ok_in, (bad_x, cy, KLT_TRACKED, 0), False)
        put(ok_in, (cx, bad_y, KLT_TRACKED, 0), False)
    put(ok_in, ok_out, True)
    put((cx, cy, 0, 0), (F32(ncols // 2), F32(nrows // 2), KLT_TRACKED, 0), True)     # integer coordinates
    for x, y, fits in edge_positions(w, ncols, nrows):                        # windows that touch each edge, on either side
        put((x, y, 1, 0), ok_out, fits)
        put(ok_in, (x, y, KLT_TRACKED, 0), fits)
    return fin, fout, want


# ------------------------------------------------------------------------------------------------ shared cases
_CASE = {}


def shifted_case():
    """320x240, 7x7, 2 levels, subsampling 4, 300 features the oracle selects on frame 1; frame 2 = frame 1 moved by LIT_SHIFT, and the
    same with gain 0.5 and offset 40 (the lit pair).  Computed once, read-only."""
    if not _CASE:
        from oracle import klt_oracle as ko
        from helpers import make_tc, params_from_tc
        from light_expected import lit_pair
        tc = make_tc(levels=2, ss=4, window=7)
        p = params_from_tc(tc)
        f1, f2 = lit_pair(320, 240, gain=1.0, offset=0.0)
        _, f2_lit = lit_pair(320, 240)
        fin = ko.select_good_features(p, f1.astype(np.float32), 300)
        pyr1, pyr2, pyr2_lit = (ko.Pyramids(p, f.astype(np.float32)) for f in (f1, f2, f2_lit))
        fin.setflags(write=False)
        _CASE.update(tc=tc, p=p, f1=f1, f2=f2, f2_lit=f2_lit, fin=fin, pyr1=pyr1, pyr2=pyr2, pyr2_lit=pyr2_lit)
    return _CASE
