"""KLT_TrackingContext -> klt_params (include/klt_gpu.h) and the three tap sets."""
import collections
import itertools
import numbers

import numpy as np

from ._abi import KltAffineParams, KltCrowdParams, KltEqualizeParams, KltFbParams, KltLightParams, KltParams
from .convolve import _computeKernels
from .klt_util import KLTComputeSmoothSigma

MAX_LEVELS = 8


def params_from_tc(tc):
    """Pack the numeric state of a tracking context.  Types follow how the reference consumes each
    value: C floats for the Cython `cdef float`s (trackFeaturesUtils.pyx:406-408), float32 for
    max_residue (compared against a numpy float32, trackFeatures.py:124), doubles elsewhere."""
    if tc.lighting_insensitive:
        # trackFeaturesUtils.pyx:434-435 raises the same exception inside the Newton loop
        raise Exception("Not implemented (the reference's switch; gain / bias tracking is tc.lightingCompensation = 'gain_bias')")
    if tc.window_width != tc.window_height:
        # the reference's patch loops are transposed for non-square windows
        raise ValueError("window_width must equal window_height")
    if tc.nPyramidLevels > MAX_LEVELS or tc.nPyramidLevels < 1:
        raise ValueError("nPyramidLevels must be in 1..%d" % MAX_LEVELS)
    p = KltParams()
    p.mindist = int(tc.mindist)
    p.window_width = int(tc.window_width)
    p.window_height = int(tc.window_height)
    p.smoothBeforeSelecting = int(bool(tc.smoothBeforeSelecting))
    p.retainTrackers = int(bool(tc.retainTrackers))
    p.nSkippedPixels = int(tc.nSkippedPixels)
    p.max_iterations = int(tc.max_iterations)
    p.nPyramidLevels = int(tc.nPyramidLevels)
    p.subsampling = int(tc.subsampling)
    p.use_max_residue = int(tc.max_residue is not None)
    p.min_determinant = float(tc.min_determinant)
    p.min_displacement = float(tc.min_displacement)
    p.step_factor = float(tc.step_factor)
    p.max_residue = float(tc.max_residue) if tc.max_residue is not None else 0.0
    p.min_eigenvalue = float(tc.min_eigenvalue)
    p.grad_sigma = float(tc.grad_sigma)
    p.smooth_sigma = float(KLTComputeSmoothSigma(tc))
    p.pyramid_sigma = float(tc.pyramid_sigma_fact * tc.subsampling)
    p.borderx = float(tc.borderx)
    p.bordery = float(tc.bordery)
    return p


def taps_from_params(p):
    """[(gauss, deriv)] for smoothing, pyramid and gradient sigma (klt_set_kernels `which` 0, 1, 2)."""
    return [_computeKernels(p.smooth_sigma), _computeKernels(p.pyramid_sigma), _computeKernels(p.grad_sigma)]


def fb_params_from_tc(tc):
    """tc.forwardBackwardCheck / tc.fb_max_error -> klt_fb_params.  Both are read with defaults: a tracking context made elsewhere (the
    reference's own class) has neither.  The check is not offered together with the affine consistency check."""
    f = KltFbParams()
    f.enabled = int(bool(getattr(tc, "forwardBackwardCheck", False)))
    f.max_error = float(getattr(tc, "fb_max_error", 1.0))
    if f.enabled and tc.affineConsistencyCheck >= 0:
        raise ValueError("forwardBackwardCheck and affineConsistencyCheck cannot both be switched on")
    if f.enabled and not f.max_error >= 0.0:
        raise ValueError("fb_max_error must be a number >= 0")
    return f


MOTION_PREDICTIONS = (None, "constant_velocity")


def motion_prediction_from_tc(tc):
    """tc.motionPrediction -> None or "constant_velocity" (read with a default: a tracking context made elsewhere has no such attribute);
    any other value is a ValueError, and so is a prediction together with the affine consistency check, which takes no prior."""
    mode = getattr(tc, "motionPrediction", None)
    if mode not in MOTION_PREDICTIONS:
        raise ValueError("tc.motionPrediction must be None or 'constant_velocity' (got {0!r})".format(mode))
    if mode is not None and tc.affineConsistencyCheck >= 0:
        raise ValueError("motionPrediction and affineConsistencyCheck cannot both be switched on")
    return mode


LIGHTING_COMPENSATIONS = (None, "gain_bias")


def light_params_from_tc(tc, guess=False, sequence=False):
    """tc.lightingCompensation -> klt_light_params: None (the default; read with one, a tracking context made elsewhere has no such
    attribute) packs mode 0, "gain_bias" mode 1, any other value is a ValueError.  The gain / bias tracker is offered on its own: a
    ValueError as well -- before any device work -- when it is switched on together with tc.forwardBackwardCheck, tc.motionPrediction,
    tc.affineConsistencyCheck >= 0, a `guess=` argument (`guess`) or KLTTrackSequence (`sequence`).  tc.lighting_insensitive, the
    reference's own switch, keeps raising "Not implemented" (params_from_tc), as the reference does."""
    mode = getattr(tc, "lightingCompensation", None)
    if not isinstance(mode, (str, type(None))) or mode not in LIGHTING_COMPENSATIONS:
        raise ValueError("tc.lightingCompensation must be None or 'gain_bias' (got {0!r})".format(mode))
    lp = KltLightParams()
    lp.mode = 0 if mode is None else 1
    if lp.mode:
        for on, what in ((bool(getattr(tc, "forwardBackwardCheck", False)), "forwardBackwardCheck"),
                         (getattr(tc, "motionPrediction", None) is not None, "motionPrediction"),
                         (getattr(tc, "affineConsistencyCheck", -1) >= 0, "affineConsistencyCheck"),
                         (bool(guess), "a guess= argument"), (bool(sequence), "KLTTrackSequence")):
            if on:
                raise ValueError("lightingCompensation and {0} cannot be used together".format(what))
    return lp


def consensus_params_from_tc(k, tc, ncols=None, nrows=None):
    """The parameters of one consensus check -- `k` a row of backend.CONSENSUS_CHECKS -- for a frame of ncols x nrows, as the row's ctypes
    struct: the switch tc.<k.switch> and tc.<k.prefix>hypotheses / seed / min_inliers / max_error (/ min_area), all read with defaults: a
    tracking context made elsewhere has none of them.  Switched off, the struct packs mode 0 and the defaults.  ValueError -- before any
    device work -- for a switch of another value, for the check together with a check of an earlier row (one consensus check per pair)
    or with tc.affineConsistencyCheck >= 0 (that check keeps per-feature state keyed on loss), and for parameters klt_set_*_params would
    refuse."""
    value = getattr(tc, k.switch, k.off)
    if k.choices is not None:
        if not isinstance(value, (str, type(None))) or value not in k.choices:
            raise ValueError("tc.{0} must be {1} (got {2!r})".format(k.switch, " or ".join(repr(c) for c in k.choices), value))
    elif not isinstance(value, (bool, np.bool_)):
        raise ValueError("tc.{0} must be True or False (got {1!r})".format(k.switch, value))
    p = k.params_type()
    p.mode = int(value is not None) if k.choices is not None else int(value)
    p.ncols, p.nrows = int(ncols or 0), int(nrows or 0)
    values = dict(k.defaults)
    if p.mode:
        from .backend import CONSENSUS_CHECKS
        for other in CONSENSUS_CHECKS[:CONSENSUS_CHECKS.index(k)]:
            theirs = getattr(tc, other.switch, other.off)
            if (theirs is not None) if other.choices is not None else theirs:
                raise ValueError("{0} and {1} cannot both be switched on".format(k.switch, other.switch))
        if getattr(tc, "affineConsistencyCheck", -1) >= 0:
            raise ValueError("{0} and affineConsistencyCheck cannot both be switched on".format(k.switch))
        for f, default in k.defaults.items():
            values[f] = type(default)(getattr(tc, k.prefix + f, default))
        if not 1 <= values["hypotheses"] <= 65536:
            raise ValueError("tc.{0}hypotheses must lie in 1 .. 65536 (got {1})".format(k.prefix, values["hypotheses"]))
        if not 0 <= values["seed"] <= 0xFFFFFFFF:
            raise ValueError("tc.{0}seed must lie in 0 .. 2**32 - 1 (got {1})".format(k.prefix, values["seed"]))
        if values["min_inliers"] < k.min_inliers_floor:
            raise ValueError("tc.{0}min_inliers must be at least {1} (got {2})".format(k.prefix, k.min_inliers_floor, values["min_inliers"]))
        floats = [f for f, default in k.defaults.items() if isinstance(default, float)]
        if not all(values[f] >= 0.0 for f in floats):       # (NaN fails)
            raise ValueError("{0} must be {1} >= 0".format(" and ".join("tc." + k.prefix + f for f in floats),
                                                           "numbers" if len(floats) > 1 else "a number"))
        if ncols is not None and not (1 <= p.ncols <= 65535 and 1 <= p.nrows <= 65535):
            raise ValueError("the {0} check takes frames of 1 .. 65535 columns and rows".format(k.title))
    for f, v in values.items():
        setattr(p, f, v)
    return p


def _consensus_check(name):
    from .backend import CONSENSUS_CHECKS
    return next(k for k in CONSENSUS_CHECKS if k.name == name)


def model_params_from_tc(tc, ncols=None, nrows=None):
    """tc.motionModelCheck (None, the default: mode 0; "affine": mode 1) / tc.model_max_error / tc.model_hypotheses / tc.model_seed /
    tc.model_min_inliers / tc.model_min_area (1.0 px^2 unless set) -> klt_model_params (consensus_params_from_tc)"""
    return consensus_params_from_tc(_consensus_check("model"), tc, ncols, nrows)


def epipolar_params_from_tc(tc, ncols=None, nrows=None):
    """tc.epipolarCheck (False, the default: mode 0; True: mode 1) / tc.epipolar_max_error / tc.epipolar_hypotheses / tc.epipolar_seed /
    tc.epipolar_min_inliers -> klt_epipolar_params (consensus_params_from_tc); never together with tc.motionModelCheck"""
    return consensus_params_from_tc(_consensus_check("epipolar"), tc, ncols, nrows)


def homography_params_from_tc(tc, ncols=None, nrows=None):
    """tc.homographyCheck (False, the default: mode 0; True: mode 1) / tc.homography_max_error / tc.homography_hypotheses /
    tc.homography_seed / tc.homography_min_inliers -> klt_homography_params (consensus_params_from_tc); never together with
    tc.motionModelCheck or tc.epipolarCheck"""
    return consensus_params_from_tc(_consensus_check("homography"), tc, ncols, nrows)


def crowd_params_from_tc(tc, ncols=None, nrows=None):
    """tc.crowdingCheck / tc.crowding_min_distance -> klt_crowd_params for a frame of ncols x nrows: False (the default) packs mode 0,
    True mode 1; crowding_min_distance None (the default) means tc.mindist.  Both are read with defaults: a tracking context made
    elsewhere has neither.  ValueError -- before any device work -- for a value that is no bool, for a distance < 1 and for the check
    together with tc.affineConsistencyCheck >= 0 (what the other checks refuse).  It goes with everything else, lighting compensation
    included: the check reads no frame."""
    on = getattr(tc, "crowdingCheck", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("tc.crowdingCheck must be True or False (got {0!r})".format(on))
    cp = KltCrowdParams()
    cp.mode = 1 if on else 0
    cp.ncols, cp.nrows = int(ncols or 0), int(nrows or 0)
    cp.min_distance = 1
    if not cp.mode:
        return cp
    if getattr(tc, "affineConsistencyCheck", -1) >= 0:
        raise ValueError("crowdingCheck and affineConsistencyCheck cannot both be switched on")
    dist = getattr(tc, "crowding_min_distance", None)
    if dist is None:
        dist = tc.mindist
    if isinstance(dist, (bool, np.bool_)) or int(dist) != dist:
        raise ValueError("tc.crowding_min_distance must be a whole number (got {0!r})".format(dist))
    if not 1 <= int(dist) <= 0x7FFFFFFF:
        raise ValueError("tc.crowding_min_distance must be at least 1 (got {0})".format(dist))
    if ncols is not None and not (1 <= cp.ncols <= 65535 and 1 <= cp.nrows <= 65535):
        raise ValueError("the crowding check takes frames of 1 .. 65535 columns and rows")
    cp.min_distance = int(dist)
    return cp


def reacquire_params_from_tc(tc):
    """tc.reacquireLost (False, the default) and, for the track identities it switches on, tc.reacquire_radius (24; None: no gate),
    tc.reacquire_max_gap (30), tc.reacquire_capacity (1024: a power of two in 1 .. 4096), tc.reacquire_max_distance (64) and
    tc.reacquire_ratio ((4, 5); None: off) -> None when the switch is off, else the six integers of klt_reacquire_params as a dict.
    All are read with defaults: a tracking context made elsewhere has none of them.  TypeError / ValueError -- before any device work
    -- for anything the library would refuse."""
    from .describeFeatures import match_params
    on = getattr(tc, "reacquireLost", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("tc.reacquireLost must be True or False (got {0!r})".format(on))
    if not on:
        return None

    def integer(name, default):
        v = getattr(tc, name, default)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
            raise TypeError("tc.{0} must be an integer (got {1!r})".format(name, v))
        return int(v)
    capacity, max_gap = integer("reacquire_capacity", 1024), integer("reacquire_max_gap", 30)
    if not (1 <= capacity <= 4096 and capacity & (capacity - 1) == 0):
        raise ValueError("tc.reacquire_capacity must be a power of two in 1 .. 4096 (got {0})".format(capacity))
    if not 0 <= max_gap <= 2 ** 31 - 1:
        raise ValueError("tc.reacquire_max_gap must be at least 0 (got {0})".format(max_gap))
    m = match_params(getattr(tc, "reacquire_max_distance", 64), getattr(tc, "reacquire_ratio", (4, 5)), True,
                     getattr(tc, "reacquire_radius", 24))
    return dict(capacity=capacity, max_gap=max_gap, max_distance=m["max_distance"], ratio_num=m["ratio_num"], ratio_den=m["ratio_den"],
                radius=m["radius"])


EQUALIZATIONS = (None, "clahe")


def equalize_params_from_tc(tc):
    """tc.equalization (None, the default: mode 0; "clahe": mode 1) / tc.clahe_tiles ((8, 8): tiles across, tiles down) /
    tc.clahe_clip_limit (3.0; None or 0: no clipping) -> klt_equalize_params, clip_q8 the limit times 256, rounded.  All three are read
    with defaults: a tracking context made elsewhere has none of them.  ValueError -- before any device work -- for another switch value
    and, with the switch on, for tiles that are no pair of integers in 1 .. 64 and for a limit that is not finite, is negative or is
    above 4096 (switched off, the struct packs mode 0 and the defaults, as the other extensions' do)."""
    mode = getattr(tc, "equalization", None)
    if mode is None:                                        # (switched off: the other two are not looked at, the struct packs the defaults)
        return KltEqualizeParams(0, 8, 8, 768)
    if not isinstance(mode, str) or mode not in EQUALIZATIONS:
        raise ValueError("tc.equalization must be None or 'clahe' (got {0!r})".format(mode))
    tiles = getattr(tc, "clahe_tiles", (8, 8))
    try:
        values = tuple(tiles)
    except TypeError:
        values = None
    if isinstance(tiles, (str, bytes)) or values is None or len(values) != 2 or not all(
            isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_)) and 1 <= v <= 64 for v in values):
        raise ValueError("tc.clahe_tiles must be (tiles_x, tiles_y), two integers in 1 .. 64 (got {0!r})".format(tiles))
    limit = getattr(tc, "clahe_clip_limit", 3.0)
    if limit is None:
        limit = 0.0
    if isinstance(limit, (bool, np.bool_)) or not isinstance(limit, numbers.Real) or not 0.0 <= float(limit) <= 4096.0:      # (NaN fails)
        raise ValueError("tc.clahe_clip_limit must be None or a number in 0 .. 4096 (got {0!r})".format(limit))
    return KltEqualizeParams(1, int(values[0]), int(values[1]), int(round(float(limit) * 256.0)))


def equalisable(ncols, nrows, tiles_x, tiles_y):
    """include/klt_gpu.h, "CLAHE ingest stage": the tile grid fits the frame and the per-pixel division is a 32-bit one"""
    if tiles_x > ncols or tiles_y > nrows:
        return False
    widest = 1
    for n, t in ((ncols, tiles_x), (nrows, tiles_y)):
        widest *= max([((k + 2) * n) // t - (k * n) // t for k in range(t - 1)] or [1])
    return widest * 255 < 2 ** 32


def _frame_class(img):
    """What the ingest stages ask of a frame: (it is a single-channel 8-bit image -- a 2-D uint8 array or a Pillow image of mode 'L' --,
    its shape (nrows, ncols) if it is one -- of any other array whatever leads its shape, which may be less --, what to call it in a
    refusal)"""
    if isinstance(img, np.ndarray):
        return img.dtype == np.uint8 and img.ndim == 2, tuple(img.shape[:2]), "a {0} array of {1} dimensions".format(img.dtype, img.ndim)
    return getattr(img, "mode", None) == "L", (img.size[1], img.size[0]), "an image of mode {0!r}".format(getattr(img, "mode", None))


def equalization_for_frames(tc, *imgs):
    """The klt_equalize_params of a call on these frames (equalize_params_from_tc).  Switched on, a ValueError that names tc.equalization
    -- before any device work -- for a frame that is not a single-channel 8-bit image (a float array, a colour or "F" Pillow image) and
    for a frame the tile grid does not fit."""
    eq = equalize_params_from_tc(tc)
    if eq.mode:
        for img in imgs:
            ok, shape, what = _frame_class(img)
            if not ok:
                raise ValueError("tc.equalization = 'clahe' takes single-channel 8-bit frames (a 2-D uint8 array or a Pillow image of "
                                 "mode 'L'), not {0}".format(what))
            nrows, ncols = shape
            if not equalisable(ncols, nrows, eq.tiles_x, eq.tiles_y):
                raise ValueError("tc.equalization = 'clahe': a {0} by {1} frame does not take tc.clahe_tiles = ({2}, {3}) (more tiles "
                                 "than pixels, or tiles too large for the 32-bit interpolation)".format(ncols, nrows, eq.tiles_x, eq.tiles_y))
    return eq


# ---------------------------------------------------------------------------------------------- remap ingest stage
_remap_serials = itertools.count(1)
_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


class KLT_RemapTable:
    """A remap for tc.remap (include/klt_gpu.h, "Remap ingest stage"): map_x, map_y -- int32 arrays of shape (nrows, ncols), for each
    pixel of the rectified frame its source position in 1/256 px -- frozen (writeable = False), with a process-wide serial number: the
    device context compares serials, not 16 MB of map, on every call.  Made by KLTCreateRemap / KLTUndistortMap."""
    __slots__ = ("map_x", "map_y", "serial")

    def __init__(self, map_x, map_y):
        ax, ay = np.asarray(map_x), np.asarray(map_y)
        for a in (ax, ay):
            if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
                raise TypeError("a remap takes integer arrays (source positions in 1/256 px), not {0}".format(a.dtype))
        if ax.ndim != 2 or ay.ndim != 2 or ax.shape != ay.shape:
            raise ValueError("a remap takes two 2-D arrays of one shape (got {0} and {1})".format(ax.shape, ay.shape))
        if not (1 <= ax.shape[0] <= 65535 and 1 <= ax.shape[1] <= 65535):
            raise ValueError("a remap takes frames of 1 .. 65535 columns and rows")
        for a in (ax, ay):
            if a.size and (int(a.min()) < _INT32_MIN or int(a.max()) > _INT32_MAX):
                raise ValueError("a remap's entries must fit 32 bits")
        self.map_x, self.map_y = (np.array(a, dtype=np.int32, order="C") for a in (ax, ay))      # (copies)
        self.map_x.setflags(write=False)
        self.map_y.setflags(write=False)
        self.serial = next(_remap_serials)

    @property
    def shape(self):
        return self.map_x.shape

    def __setattr__(self, name, value):
        if hasattr(self, "serial"):                         # (the serial is set last)
            raise AttributeError("a KLT_RemapTable is immutable")
        object.__setattr__(self, name, value)


def KLTCreateRemap(map_x, map_y):
    """Not in the reference: a KLT_RemapTable from two 2-D integer arrays of one shape (nrows, ncols) -- for each pixel of the frame the
    tracker is to see, the position in the incoming frame it is read from, in 1/256 px, pixel centres at integers; any int32 value is
    legal (positions outside the frame read the nearest edge pixel).  The arrays are copied.  TypeError for float arrays, ValueError for
    shapes that differ."""
    return KLT_RemapTable(map_x, map_y)


def _distort(x, y, dist):
    """forward Brown-Conrady: normalised pinhole coordinates -> normalised distorted coordinates"""
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return (x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x),
            y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)


def _camera(matrix, what):
    k = np.asarray(matrix, np.float64)
    if k.shape != (3, 3) or not np.isfinite(k).all() or k[0, 0] == 0.0 or k[1, 1] == 0.0:
        raise ValueError("{0} must be a finite 3 x 3 matrix with non-zero focal lengths".format(what))
    return k[0, 0], k[1, 1], k[0, 2], k[1, 2]


def KLTUndistortMap(ncols, nrows, camera_matrix, dist_coeffs, new_camera_matrix=None):
    """Not in the reference: the KLT_RemapTable that undoes a lens's distortion.  Host numpy in FP64, the forward Brown-Conrady model
    with coefficients (k1, k2, p1, p2[, k3]) -- no iteration: a pixel (u, v) of the rectified frame under new_camera_matrix (None: the
    camera matrix) is normalised, x = (u - cx') / fx', y = (v - cy') / fy'; distorted, r2 = x x + y y, radial = 1 + k1 r2 + k2 r2^2 +
    k3 r2^3, xd = x radial + 2 p1 x y + p2 (r2 + 2 x x), yd = y radial + p1 (r2 + 2 y y) + 2 p2 x y; and projected with the camera
    matrix, us = fx xd + cx, vs = fy yd + cy (the matrices' focal lengths and principal point are read, a skew is not).  Entries are
    rint(256 us), rint(256 vs), clipped to int32."""
    ncols, nrows = int(ncols), int(nrows)
    if not (1 <= ncols <= 65535 and 1 <= nrows <= 65535):
        raise ValueError("a remap takes frames of 1 .. 65535 columns and rows")
    dist = np.asarray(dist_coeffs, np.float64).ravel()
    if dist.size not in (4, 5) or not np.isfinite(dist).all():
        raise ValueError("dist_coeffs must be (k1, k2, p1, p2) or (k1, k2, p1, p2, k3), finite")
    dist = np.concatenate([dist, np.zeros(5 - dist.size)])
    fx, fy, cx, cy = _camera(camera_matrix, "camera_matrix")
    nfx, nfy, ncx, ncy = (fx, fy, cx, cy) if new_camera_matrix is None else _camera(new_camera_matrix, "new_camera_matrix")
    v, u = np.mgrid[0:nrows, 0:ncols].astype(np.float64)
    xd, yd = _distort((u - ncx) / nfx, (v - ncy) / nfy, dist)
    entries = [np.clip(np.rint(256.0 * s), _INT32_MIN, _INT32_MAX).astype(np.int64) for s in (fx * xd + cx, fy * yd + cy)]
    return KLT_RemapTable(entries[0], entries[1])


def _table(table):
    if not isinstance(table, KLT_RemapTable):
        raise TypeError("expected a KLT_RemapTable (KLTCreateRemap, KLTUndistortMap), got {0!r}".format(type(table).__name__))
    return table


def KLTRemapValidMask(table, margin=0):
    """Not in the reference: a uint8 array for tc.selectionMask -- 1 where the map's (unclamped) source position lies inside the frame
    by `margin` px on both axes, 0 where the remapped frame shows replicated edge pixels (or comes within `margin` of them)."""
    t = _table(table)
    nrows, ncols = t.shape
    m = int(round(float(margin) * 256.0))
    ok = (t.map_x >= m) & (t.map_x <= (ncols - 1) * 256 - m) & (t.map_y >= m) & (t.map_y <= (nrows - 1) * 256 - m)
    return ok.astype(np.uint8)


def KLTRemapSourcePositions(table, x, y):
    """Not in the reference: where positions of the rectified frame (what the tracker reports with tc.remap set) lie in the incoming
    frame -- the map read bilinearly at (x, y) in FP64, in px; positions outside the frame read the map's edge.  At whole positions
    these are the map's entries over 256."""
    t = _table(table)
    nrows, ncols = t.shape
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    xc, yc = np.clip(x, 0.0, ncols - 1.0), np.clip(y, 0.0, nrows - 1.0)
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, ncols - 1), np.minimum(y0 + 1, nrows - 1)
    ax, ay = xc - x0, yc - y0
    out = []
    for m in (t.map_x, t.map_y):
        m = m.astype(np.float64)
        out.append(((1.0 - ax) * (1.0 - ay) * m[y0, x0] + ax * (1.0 - ay) * m[y0, x1] + (1.0 - ax) * ay * m[y1, x0] + ax * ay * m[y1, x1]) / 256.0)
    return out[0], out[1]


def remap_from_tc(tc):
    """tc.remap (None, the default: the stage is off) -> the KLT_RemapTable of the call, or None.  Read with a default: a tracking context
    made elsewhere has no such attribute.  TypeError -- before any device work -- for anything else."""
    table = getattr(tc, "remap", None)
    if table is not None and not isinstance(table, KLT_RemapTable):
        raise TypeError("tc.remap must be None or a KLT_RemapTable (KLTCreateRemap, KLTUndistortMap), got {0!r}".format(type(table).__name__))
    return table


def remap_for_frames(tc, *imgs):
    """The KLT_RemapTable of a call on these frames (remap_from_tc), or None.  Switched on, a ValueError that names tc.remap -- before any
    device work -- for a frame that is not a single-channel 8-bit image and for a frame whose shape is not the table's."""
    table = remap_from_tc(tc)
    if table is not None:
        for img in imgs:
            ok, shape, what = _frame_class(img)
            if not ok:
                raise ValueError("tc.remap takes single-channel 8-bit frames (a 2-D uint8 array or a Pillow image of mode 'L'), not {0}".format(what))
            if shape != table.shape:
                raise ValueError("tc.remap: the frame is {0} by {1}, the table {2} by {3}".format(shape[1], shape[0], table.shape[1], table.shape[0]))
    return table


PostTrack = collections.namedtuple("PostTrack", "consensus crowd quality")
NO_POST_TRACK = PostTrack((), None, False)


def post_track_from_tc(tc, ncols=None, nrows=None):
    """What follows every tracker launch of a call on this tracking context, as Context.post_track_async enqueues it (DESIGN.md "what a
    post-track stage is made of"): `consensus` ((row of backend.CONSENSUS_CHECKS, its parameter struct), ...) of the checks that are
    switched on (never two), `crowd` the klt_crowd_params of tc.crowdingCheck or None, `quality` tc.trackQuality.  Every ValueError of
    consensus_params_from_tc (the rows in their order) and then of crowd_params_from_tc is raised here: without a frame size this is
    the refusal pass an entry point runs before it touches the device, with one what it then uses."""
    from .backend import CONSENSUS_CHECKS
    consensus = ()
    for k in CONSENSUS_CHECKS:
        p = consensus_params_from_tc(k, tc, ncols, nrows)
        if p.mode:
            consensus += ((k, p),)
    crowd = crowd_params_from_tc(tc, ncols, nrows)
    return PostTrack(consensus, crowd if crowd.mode else None, bool(getattr(tc, "trackQuality", False)))


def age_records(age, n):
    """The `age=` argument of KLTTrackFeatures -> None, or n klt_crowd records whose age column holds it: an (n,) integer array-like (the
    age column of the last call's tc.crowding_last).  ValueError for another shape or for values that are no 32-bit integers."""
    if age is None:
        return None
    a = np.asarray(age)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise ValueError("age must be an integer array of shape ({0},) (got {1} of {2})".format(n, a.dtype, a.shape))
    if n and (a.min() < -0x80000000 or a.max() > 0x7FFFFFFF):
        raise ValueError("age must hold 32-bit integers")
    rec = np.zeros((n, 4), np.int32)
    rec[:, 0] = a
    return rec


def guess_records(guess, n, affine=False):
    """The `guess=` argument of KLTTrackFeatures -> None, or n klt_feat records: an (n, 2) array-like of predicted frame-2 positions,
    a row with a NaN = no guess for that feature (val -1; a row with an infinity is sent as it is and does not count either).  ValueError
    for another shape, and for a guess together with the affine consistency check -- before any device work."""
    if guess is None:
        return None
    if affine:
        raise ValueError("guess= and affineConsistencyCheck cannot be used together: the affine check takes no prior")
    g = np.asarray(guess, np.float32)
    if g.shape != (n, 2):
        raise ValueError("guess must be an (n, 2) array of predicted positions for the {0} features (got shape {1})".format(n, g.shape))
    from .backend import FEAT_DTYPE
    rec = np.zeros(n, FEAT_DTYPE)
    rec["x"], rec["y"] = g[:, 0], g[:, 1]
    rec["val"] = np.where(np.isnan(g).any(axis=1), -1, 0)
    return rec


def selection_mask_from_tc(tc, ncols=None, nrows=None):
    """tc.selectionMask -> None, or the [nrows][ncols] uint8 array klt_set_select_mask takes (0 = never a candidate).  Read with a default:
    a tracking context made elsewhere (the reference's own class) has no such attribute.  Accepted: a 2-D numpy array of bool or of any
    integer type (non-zero = allowed), or a Pillow image of mode "L" or "1"; anything else is a TypeError, a shape other than the image's
    (when `ncols` / `nrows` are given) a ValueError -- both before any device work.  A C-contiguous uint8 or bool array is used as it is
    (no copy), so what is handed out must be looked at before the caller's next statement runs."""
    mask = getattr(tc, "selectionMask", None)
    if mask is None:
        return None
    if not isinstance(mask, np.ndarray):
        if getattr(mask, "mode", None) not in ("L", "1") or not hasattr(mask, "size"):
            raise TypeError("tc.selectionMask must be a 2-D numpy array of bool or integers, or a Pillow image of mode 'L' or '1' "
                            "(got {0})".format(type(mask).__name__ if not hasattr(mask, "mode") else "an image of mode %r" % (mask.mode,)))
        mask = np.asarray(mask)
    if mask.dtype != np.bool_ and not np.issubdtype(mask.dtype, np.integer):
        raise TypeError("tc.selectionMask must hold bool or integers, not {0}".format(mask.dtype))
    if mask.ndim != 2:
        raise ValueError("tc.selectionMask must be 2-D ({0} dimensions)".format(mask.ndim))
    if ncols is not None and mask.shape != (nrows, ncols):
        raise ValueError("tc.selectionMask is {0} by {1}, the image {2} by {3}".format(mask.shape[1], mask.shape[0], ncols, nrows))
    if mask.dtype == np.bool_ or mask.dtype.itemsize == 1:
        return np.ascontiguousarray(mask).view(np.uint8)            # (int8: a non-zero value is a non-zero byte)
    return (mask != 0).view(np.uint8)


def select_grid_from_tc(tc):
    """tc.selectionGrid -> None, or the (cell_width, cell_height, max_per_cell) tuple of ints klt_set_select_grid takes.  Read with a
    default, like tc.selectionMask.  TypeError for a value that is not a sequence of three integers (a bool is not one), ValueError for a
    cell side below 1 or max_per_cell outside 1 .. 65535 -- both before any device work."""
    grid = getattr(tc, "selectionGrid", None)
    if grid is None:
        return None
    import numbers
    try:
        values = tuple(grid)
    except TypeError:
        values = None
    if isinstance(grid, (str, bytes)) or values is None or len(values) != 3 or not all(
            isinstance(v, numbers.Integral) and not isinstance(v, (bool, np.bool_)) for v in values):
        raise TypeError("tc.selectionGrid must be None or (cell_width, cell_height, max_per_cell), three integers (got {0!r})".format(grid))
    cw, ch, q = (int(v) for v in values)
    if cw < 1 or ch < 1 or cw > 2 ** 31 - 1 or ch > 2 ** 31 - 1:
        raise ValueError("tc.selectionGrid: cell_width and cell_height must be at least 1 (got {0} x {1})".format(cw, ch))
    if not 1 <= q <= 65535:
        raise ValueError("tc.selectionGrid: max_per_cell must lie in 1 .. 65535 (got {0})".format(q))
    return cw, ch, q


def affine_params_from_tc(tc):
    """klt.py:67-73 -> klt_affine_params (mode -1 = consistency check off)."""
    a = KltAffineParams()
    a.mode = int(tc.affineConsistencyCheck)
    a.window_width = int(tc.affine_window_width)
    a.window_height = int(tc.affine_window_height)
    a.max_iterations = int(tc.affine_max_iterations)
    a.max_residue = float(tc.affine_max_residue)
    a.min_displacement = float(tc.affine_min_displacement)
    a.max_displacement_differ = float(tc.affine_max_displacement_differ)
    return a
