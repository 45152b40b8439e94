"""Thin object wrapper over the C ABI (include/klt_gpu.h) -- one `Context` per device.

Everything numeric happens behind the ABI in hand-written HIP kernels; this module only
marshals numpy buffers and keeps the tracking-context parameters in sync.  There is no
CPU fallback: creating a Context without a usable MI355X raises KltBackendError.
"""
import collections
import ctypes as C
import os as _os
import threading

import numpy as np

from ._abi import (KLT_MAX_LEVELS, KltAffineRec, KltFbParams, KltLightParams, KltSelectGrid, KltBackendError, KltCommTimeout, KltOutOfMemory, KltFeat, KltKernelTime, KltParams,
                   KltBankEntry, KltIdent, KltReacquireParams, KltReacquireState,
                   KltCrowd, KltCrowdParams, KltDescriptor, KltDescriptorParams, KltMatch, KltMatchParams, KltEqualizeParams, KltEpipolarModel, KltEpipolarParams, KltHomographyModel, KltHomographyParams, KltModelParams, KltMotionModel, KltQuality, KltTrackStats, load_library)
from .params import affine_params_from_tc, equalize_params_from_tc, fb_params_from_tc, light_params_from_tc, params_from_tc, remap_from_tc, taps_from_params

FEAT_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("val", np.int32), ("aux", np.int32)])
assert FEAT_DTYPE.itemsize == C.sizeof(KltFeat)
AFFINE_DTYPE = np.dtype([("aff_x", np.float32), ("aff_y", np.float32), ("Axx", np.float32), ("Ayx", np.float32),
                         ("Axy", np.float32), ("Ayy", np.float32), ("valid", np.int32), ("pad", np.int32)])
assert AFFINE_DTYPE.itemsize == C.sizeof(KltAffineRec)
# a quality record (klt_quality; klt_track_quality*): it lives in a feature buffer, and Python reads that buffer's records through this view
QUALITY_DTYPE = np.dtype([("residue", np.float32), ("ncc", np.float32), ("min_eig", np.float32), ("val", np.int32)])
assert QUALITY_DTYPE.itemsize == C.sizeof(KltQuality) == FEAT_DTYPE.itemsize

# a motion model (klt_motion_model; klt_motion_check*): one record in a feature buffer of five klt_feat records
MODEL_DTYPE = np.dtype([("nxx", np.float64), ("nxy", np.float64), ("ntx", np.float64), ("nyx", np.float64), ("nyy", np.float64),
                        ("nty", np.float64), ("d", np.float64), ("valid", np.int32), ("n_candidates", np.int32), ("n_inliers", np.int32),
                        ("hypothesis", np.int32), ("hypothesis_inliers", np.int32), ("pad", np.int32)])
assert MODEL_DTYPE.itemsize == C.sizeof(KltMotionModel) == 5 * FEAT_DTYPE.itemsize
# an epipolar model (klt_epipolar_model; klt_epipolar_check*): one record in a feature buffer of six klt_feat records
EPIPOLAR_DTYPE = np.dtype([("f", np.float64, (9,)), ("valid", np.int32), ("n_candidates", np.int32), ("n_inliers", np.int32),
                           ("hypothesis", np.int32), ("hypothesis_inliers", np.int32), ("pad", np.int32)])
assert EPIPOLAR_DTYPE.itemsize == C.sizeof(KltEpipolarModel) == 6 * FEAT_DTYPE.itemsize
# a homography model (klt_homography_model; klt_homography_check*): likewise one record in a feature buffer of six klt_feat records
HOMOGRAPHY_DTYPE = np.dtype([("h", np.float64, (9,)), ("valid", np.int32), ("n_candidates", np.int32), ("n_inliers", np.int32),
                             ("hypothesis", np.int32), ("hypothesis_inliers", np.int32), ("pad", np.int32)])
assert HOMOGRAPHY_DTYPE.itemsize == C.sizeof(KltHomographyModel) == 6 * FEAT_DTYPE.itemsize
# one crowd record per feature (klt_crowd; klt_crowd_check*): age = the consecutive steps the slot has been tracked, winner = the record a
# crowded one merged into (-1 otherwise), val 0 non-candidate / 1 kept / 2 crowded; they live in feature buffers like quality records
CROWD_DTYPE = np.dtype([("age", np.int32), ("winner", np.int32), ("val", np.int32), ("pad", np.int32)])
assert CROWD_DTYPE.itemsize == C.sizeof(KltCrowd) == FEAT_DTYPE.itemsize
# a descriptor (klt_descriptor; klt_describe*): one record in three klt_feat records of a feature buffer; a match record (klt_match;
# klt_match*): one klt_feat record per query
DESCRIPTOR_DTYPE = np.dtype([("bits", np.uint32, (8,)), ("val", np.int32), ("orientation", np.int32), ("cx", np.int32), ("cy", np.int32)])
assert DESCRIPTOR_DTYPE.itemsize == C.sizeof(KltDescriptor) == 3 * FEAT_DTYPE.itemsize
MATCH_DTYPE = np.dtype([("train", np.int32), ("distance", np.int32), ("second", np.int32), ("val", np.int32)])
assert MATCH_DTYPE.itemsize == C.sizeof(KltMatch) == FEAT_DTYPE.itemsize
# an ident record (klt_ident; klt_reacquire_*): one klt_feat record per slot, val 0 no track / 1 continued / 2 new / 3 re-acquired; an
# entry of the bank of lost tracks and the counters, as the two synchronous diagnostics return them
IDENT_DTYPE = np.dtype([("id", np.int32), ("gap", np.int32), ("distance", np.int32), ("val", np.int32)])
assert IDENT_DTYPE.itemsize == C.sizeof(KltIdent) == FEAT_DTYPE.itemsize
BANK_DTYPE = np.dtype([("d", DESCRIPTOR_DTYPE), ("id", np.int32), ("last_seen", np.int32), ("valid", np.int32), ("pad", np.int32)])
assert BANK_DTYPE.itemsize == C.sizeof(KltBankEntry) == 64
REACQUIRE_STATE_DTYPE = np.dtype([(k, np.int32) for k in ("k", "h", "next_id", "valid", "fresh", "lost")])
assert REACQUIRE_STATE_DTYPE.itemsize == C.sizeof(KltReacquireState)

SELECTING_ALL = 1
REPLACING_SOME = 2
# the reference-shaped API's tracker reads and writes its pinned record arrays in place (klt_featbuf_map_host); KLT_MAP_RECORDS=0 in
# the environment goes back to one copy command each way
MAP_RECORDS = _os.environ.get("KLT_MAP_RECORDS", "1") != "0"
# Feature-buffer ids: every id the Python layer uses, and the ones the library keeps for itself, in this one table.
_FB_LIBRARY = (65530, 65531, 65532, 65534, 65535)   # staging buffers of the library's synchronous entry points (klt_track*, klt_select, ...)
_FB_API_SELECT = 65533               # the selection list of the reference-shaped API while its records are not mapped (MAP_RECORDS)
_FB_API_IN, _FB_API_OUT = 65526, 65527               # the tracker's two lists in a KLTTrackFeatures call
_FB_API_BACK = 65528                 # backward records of a forward-backward call of that API (device memory, read back on request)
_FB_API_GUESS = 65529                # predicted positions of a KLTTrackFeatures(..., guess=) call
_FB_GUESS = 65525                    # KLTTrackSequence: the constant-velocity guesses of the step being enqueued (tc.motionPrediction)
# KLTTrackSequence's record tables (trackSequence._RecordTable): chunk ci of a table is buffer base + ci * (FB_CHUNK + 1), its FB_CHUNK rows the
# ids behind it.  The feature table ends the call at _MAX_FRAMES; the others follow its rows.
FB_CHUNK = 64
_FB_TABLE = 60000                    # the feature lists, one row per frame
_FBQ_TABLE = 54000                   # tc.trackQuality: quality records
_FBM_TABLE, _FBE_TABLE, _FBH_TABLE = 48000, 42000, 36000        # tc.motionModelCheck, tc.epipolarCheck, tc.homographyCheck: a model record per frame
_FBC_TABLE = 30000                   # tc.crowdingCheck: crowd records
_MAX_FRAMES = 65535 - (_FB_TABLE + 1)
# ... and the buffers of the same records in a KLTTrackFeatures call: the last id below the next table up
_FB_API_QUALITY, _FB_API_MODEL, _FB_API_EPIPOLAR, _FB_API_HOMOGRAPHY, _FB_API_CROWD = 59999, 53999, 47999, 41999, 35999
_FB_API_CROWD_PREV = 29999           # ... and the ages the caller handed in (age=)
# KLTDescribeFeatures: the list and its descriptors; KLTMatchDescriptors: the two descriptor sets and the match records
_FB_API_DESCRIBE_IN, _FB_API_DESCRIBE = 29998, 29997
_FB_API_MATCH_QUERY, _FB_API_MATCH_TRAIN, _FB_API_MATCH = 29996, 29995, 29994
# track identities: KLTUpdateIdentities' list and its two alternating ident rows; the two descriptor buffers the library keeps for
# itself (klt_reacquire_*: P and Q); KLTTrackSequence's table of ident rows (tc.reacquireLost)
_FB_API_IDENT_IN, _FB_API_IDENT = 29993, (29992, 29989)
_FB_LIBRARY_REACQUIRE = (29990, 29991)
_FBI_TABLE = 24000
# no id of a table that has grown as far as it can is a single buffer or an id of another table, and all of them lie below 65535
_ids = [base + i for base in (_FB_TABLE, _FBQ_TABLE, _FBM_TABLE, _FBE_TABLE, _FBH_TABLE, _FBC_TABLE, _FBI_TABLE)
        for i in range(_MAX_FRAMES // (FB_CHUNK + 1) * (FB_CHUNK + 1))]
assert max(_ids) < 65535 and len(set(_ids + list(_FB_LIBRARY + _FB_LIBRARY_REACQUIRE + _FB_API_IDENT + (
    _FB_API_SELECT, _FB_API_IN, _FB_API_OUT, _FB_API_BACK, _FB_API_GUESS, _FB_GUESS, _FB_API_QUALITY, _FB_API_MODEL, _FB_API_EPIPOLAR,
    _FB_API_HOMOGRAPHY, _FB_API_CROWD, _FB_API_CROWD_PREV, _FB_API_DESCRIBE_IN, _FB_API_DESCRIBE, _FB_API_MATCH_QUERY, _FB_API_MATCH_TRAIN,
    _FB_API_MATCH, _FB_API_IDENT_IN)))) == len(_ids) + 27
del _ids

# The three consensus checks over feature lists (DESIGN.md "what a consensus check is made of"), one row each: everything params.py,
# the Context methods below, KLTTrackFeatures and KLTTrackSequence know of a check.  The order counts: a check refuses to be switched on
# beside one of an earlier row (params.consensus_params_from_tc), and the entry points go through the rows in this order.
#   name, title        the check in identifiers (klt_set_<name>_params, Context.<name>_download) and in messages
#   c_check            klt_<c_check>_check, ..._async, ..._batch_async, ..._path
#   switch, choices    the tracking context's switch: one of `choices` (the first is off), or a bool where `choices` is None
#   prefix, defaults   tc.<prefix><field> for every field of `defaults`, read with these defaults; min_inliers_floor: the smallest allowed
#   params_type, model_type, dtype, records    the ctypes structs, and the model record as numpy sees it: `records` feature records
#   fb_api, fb_table   the model record's feature buffer in a KLTTrackFeatures call; the base of KLTTrackSequence's table of them
#   last, ft, summary  tc.<last> after KLTTrackFeatures (summary(record), or the record itself); <ft> of KLTTrackSequence's result
ConsensusCheck = collections.namedtuple("ConsensusCheck", "name title c_check switch choices prefix defaults min_inliers_floor params_type "
                                        "model_type dtype records fb_api fb_table last ft summary")
ConsensusCheck.off = property(lambda k: k.choices[0] if k.choices is not None else False)
CONSENSUS_CHECKS = (
    ConsensusCheck("model", "motion-model", "motion", "motionModelCheck", (None, "affine"), "model_",
                   dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0, min_area=1.0), 3, KltModelParams, KltMotionModel, MODEL_DTYPE, 5,
                   _FB_API_MODEL, _FBM_TABLE, "model_last", "models", lambda record: model_summary(record)),
    ConsensusCheck("epipolar", "epipolar", "epipolar", "epipolarCheck", None, "epipolar_",
                   dict(hypotheses=512, seed=0, min_inliers=16, max_error=1.0), 8, KltEpipolarParams, KltEpipolarModel, EPIPOLAR_DTYPE, 6,
                   _FB_API_EPIPOLAR, _FBE_TABLE, "epipolar_last", "epipolar", None),
    ConsensusCheck("homography", "homography", "homography", "homographyCheck", None, "homography_",
                   dict(hypotheses=256, seed=0, min_inliers=8, max_error=1.0), 4, KltHomographyParams, KltHomographyModel, HOMOGRAPHY_DTYPE, 6,
                   _FB_API_HOMOGRAPHY, _FBH_TABLE, "homography_last", "homography", None),
)
_MODEL_CHECK, _EPIPOLAR_CHECK, _HOMOGRAPHY_CHECK = CONSENSUS_CHECKS
assert all(k.dtype.itemsize == C.sizeof(k.model_type) == k.records * FEAT_DTYPE.itemsize for k in CONSENSUS_CHECKS)
PostTrackTargets = collections.namedtuple("PostTrackTargets", "model crowd_prev crowd quality")       # (Context.post_track_async)


def _dp(a):
    return (C.c_double * len(a))(*a)


def _columns(pairs, count):
    """the first `count` columns of a `pairs` list as c_int arrays: what a batched entry point takes"""
    return [(C.c_int * len(pairs))(*[p[k] for p in pairs]) for k in range(count)]


class Context:
    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.klt_create(int(device), C.byref(h))
        if rc != 0:
            msg = self._lib.klt_last_error(None)
            raise KltBackendError("klt_create(device=%d) failed (%d): %s" % (device, rc, (msg or b"").decode()))
        self._h = h
        self.device = int(device)
        self._params_key = None
        self._consensus_keys = {}            # CONSENSUS_CHECKS: name -> the parameter bytes the library holds
        # One context = one HIP stream set + one set of pinned record buffers: never two host threads inside it at a time
        # (include/klt_gpu.h, "Threads").  The reference-shaped API holds this lock for the length of a KLT* call; callers that
        # drive a Context directly from several threads take it themselves (`with ctx.lock:`) or give each thread its own.
        self.lock = threading.RLock()
        self._deferred = collections.deque()          # releases asked for by finalizers that could not get the lock at once

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_h", None):
            self._lib.klt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            msg = self._lib.klt_last_error(self._h)
            kind = KltCommTimeout if rc == -5 else (KltOutOfMemory if rc == -4 else KltBackendError)      # KLT_ERR_TIMEOUT, KLT_ERR_NOMEM
            raise kind("libkltgpu error %d: %s" % (rc, (msg or b"").decode()))
        return rc

    def sync(self):
        self._check(self._lib.klt_sync(self._h))

    def stream_handle(self):
        return self._lib.klt_stream_handle(self._h)

    # ---------------------------------------------------------------- parameters
    def set_params(self, p):
        """p: KltParams.  Taps for the three sigmas are generated on the host (convolve.py:27-93)."""
        key = bytes(p)
        if key == self._params_key:
            return
        self._check(self._lib.klt_set_params(self._h, C.byref(p)))
        # taps depend on the three sigmas only: a change of mindist / max_residue / ... must not touch them (the library
        # invalidates resident pyramids when taps change -- sequentialMode keeps tc.pyramid_last across such changes)
        sig = (p.smooth_sigma, p.pyramid_sigma, p.grad_sigma)
        if sig != getattr(self, "_sigma_key", None):
            for which, (g, d) in enumerate(taps_from_params(p)):
                self._check(self._lib.klt_set_kernels(self._h, which, _dp(g), len(g), _dp(d), len(d)))
            self._sigma_key = sig
        self._params_key = key
        self.params = p

    def configured_for(self, tc):
        """True when configure(tc) would change nothing that voids resident pyramids"""
        return bytes(params_from_tc(tc)) == self._params_key

    def configure(self, tc):
        light = light_params_from_tc(tc)                 # (ValueError for a combination that is not offered, before anything is set)
        eq = equalize_params_from_tc(tc)                 # (likewise for tc.equalization and its parameters)
        remap = remap_from_tc(tc)                        # (likewise for tc.remap)
        self.set_params(params_from_tc(tc))
        self.set_equalize_params(eq, only_if_on=True)
        self.sync_remap(remap)
        self.set_light_params(light)
        self.set_affine_params(affine_params_from_tc(tc))
        fb = fb_params_from_tc(tc)
        if fb.enabled:
            self.set_fb_params(fb)

    # ------------------------------------------------ CLAHE ingest stage (klt_set_equalize_params)
    def set_equalize_params(self, eq=None, only_if_on=False, **kw):
        """klt_set_equalize_params: `eq` a KltEqualizeParams, or its fields by name (mode, tiles_x, tiles_y, clip_q8; the defaults: off,
        8 x 8 tiles, clip limit 3.0).  Sent when it differs from what the library holds.  `only_if_on`: a struct with mode 0 is sent only
        to switch off an equalisation that is on -- a context that never had it on gets no call at all."""
        if eq is None:
            eq = KltEqualizeParams(int(kw.pop("mode", 0)), int(kw.pop("tiles_x", 8)), int(kw.pop("tiles_y", 8)), int(kw.pop("clip_q8", 768)))
            assert not kw, kw
        key = bytes(eq)
        held = getattr(self, "_equalize_key", None)
        if only_if_on and not eq.mode and (held is None or not KltEqualizeParams.from_buffer_copy(held).mode):
            return
        if key != held:
            self._check(self._lib.klt_set_equalize_params(self._h, C.byref(eq)))
            self._equalize_key = key

    def equalize(self, img, ncols=None):
        """klt_equalize_u8: the equalised frame of a 2-D uint8 array under the context's tiles and clip limit, whatever its mode.
        `ncols`: the frame is the first ncols columns of `img` (whose width is then the pitch)"""
        a = np.ascontiguousarray(img)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("expected a 2-D uint8 image")
        nrows, pitch = a.shape
        out = np.empty((nrows, pitch if ncols is None else int(ncols)), np.uint8)
        self._check(self._lib.klt_equalize_u8(self._h, a.ctypes.data, out.shape[1], nrows, pitch, out.ctypes.data))
        return out

    def download_equalized(self, slot, ncols, nrows):
        """klt_download_equalized_u8: the equalised frame the slot's last build read"""
        out = np.empty((nrows, ncols), np.uint8)
        self._check(self._lib.klt_download_equalized_u8(self._h, slot, out.ctypes.data))
        return out

    def equalize_path(self):
        """klt_equalize_path: 1 if the last build enqueued equalisation launches, 0 if not (a diagnostic)"""
        return self._check(self._lib.klt_equalize_path(self._h))

    # ------------------------------------------------ remap ingest stage (klt_set_remap)
    def set_remap(self, map_x=None, map_y=None):
        """klt_set_remap: two int32 arrays of one 2-D shape (nrows, ncols), source positions in 1/256 px; None, None switches the stage off"""
        if map_x is None and map_y is None:
            self._check(self._lib.klt_set_remap(self._h, None, None, 0, 0))
        elif map_x is None or map_y is None:
            raise ValueError("both planes of the map, or neither")
        else:
            mx, my = np.ascontiguousarray(map_x, np.int32), np.ascontiguousarray(map_y, np.int32)
            if mx.ndim != 2 or mx.shape != my.shape:
                raise ValueError("expected two 2-D arrays of one shape")
            self._check(self._lib.klt_set_remap(self._h, mx.ctypes.data, my.ctypes.data, mx.shape[1], mx.shape[0]))
        self._remap_set, self._remap_serial = map_x is not None, None      # (a map sent by hand is no table's)

    def sync_remap(self, table):
        """tc.remap as the call found it (params.remap_from_tc: a KLT_RemapTable or None): the map goes to the library only when the
        table's serial is not the one the context holds, None only to switch off a map that is set -- a context that never had one gets
        no call at all."""
        if table is None:
            if getattr(self, "_remap_set", False):
                self.set_remap()
        elif not getattr(self, "_remap_set", False) or getattr(self, "_remap_serial", None) != table.serial:
            self.set_remap(table.map_x, table.map_y)
            self._remap_serial = table.serial

    def remap(self, img, ncols=None):
        """klt_remap_u8: the remapped frame of a 2-D uint8 array under the context's map.  `ncols`: the frame is the first ncols columns
        of `img` (whose width is then the pitch)"""
        a = np.ascontiguousarray(img)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError("expected a 2-D uint8 image")
        nrows, pitch = a.shape
        out = np.empty((nrows, pitch if ncols is None else int(ncols)), np.uint8)
        self._check(self._lib.klt_remap_u8(self._h, a.ctypes.data, out.shape[1], nrows, pitch, out.ctypes.data))
        return out

    def download_remapped(self, slot, ncols, nrows):
        """klt_download_remapped_u8: the remapped frame the slot's last build read"""
        out = np.empty((nrows, ncols), np.uint8)
        self._check(self._lib.klt_download_remapped_u8(self._h, slot, out.ctypes.data))
        return out

    def remap_path(self):
        """klt_remap_path: 1 if the last build enqueued a remap launch, 0 if not (a diagnostic)"""
        return self._check(self._lib.klt_remap_path(self._h))

    # ------------------------------------------------ gain / bias tracking (klt_set_light_params)
    def set_light_params(self, lp=None, mode=None):
        """klt_set_light_params: `lp` a KltLightParams, or mode alone (0 off, 1 gain + bias).  While mode 1 is set, track / track_async /
        track_batch_async run the gain / bias kernels and every other tracker entry point is refused."""
        if lp is None:
            lp = KltLightParams(int(mode))
        key = bytes(lp)
        if key != getattr(self, "_light_key", None):
            self._check(self._lib.klt_set_light_params(self._h, C.byref(lp)))
            self._light_key = key

    def track_light_path(self):
        """klt_track_light_path: 0 no lighting launch yet, 1 wave kernel, 2 quad kernel (the last launch with mode 1; a diagnostic)"""
        return self._check(self._lib.klt_track_light_path(self._h))

    # ------------------------------------------- forward-backward consistency check
    def set_fb_params(self, fb=None, max_error=None):
        """klt_set_fb_params: `fb` a KltFbParams, or max_error alone"""
        if fb is None:
            fb = KltFbParams(1, float(max_error))
        key = bytes(fb)
        if key != getattr(self, "_fb_key", None):
            self._check(self._lib.klt_set_fb_params(self._h, C.byref(fb)))
            self._fb_key = key

    def track_fb(self, slot1, slot2, fl, want_back=False):
        """klt_track_fb on a copy: (records after the check, number still tracked[, backward records])."""
        fl = np.ascontiguousarray(fl, FEAT_DTYPE).copy()
        back = np.empty(len(fl), FEAT_DTYPE) if want_back else None
        k = C.c_int()
        self._check(self._lib.klt_track_fb(self._h, slot1, slot2, fl.ctypes.data, back.ctypes.data if want_back else None, len(fl),
                                           C.byref(k)))
        return (fl, k.value, back) if want_back else (fl, k.value)

    def track_fb_async(self, slot1, slot2, fb_in, fb_out, n, fb_back=-1):
        self._check(self._lib.klt_track_fb_async(self._h, slot1, slot2, fb_in, fb_out, n, fb_back))

    def track_fb_batch_async(self, pairs, n):
        """pairs: [(slot1, slot2, fb_in, fb_out[, fb_back]), ...] -- one forward-backward launch for all of them; without any fb_back
        no backward records are kept."""
        cols = _columns(pairs, 4)
        back = None
        if any(len(p) > 4 for p in pairs):
            back = (C.c_int * len(pairs))(*[p[4] if len(p) > 4 else -1 for p in pairs])
        self._check(self._lib.klt_track_fb_batch_async(self._h, cols[0], cols[1], cols[2], cols[3], back, len(pairs), n))

    # ------------------------------------------------ motion prior (klt_track_guess*, klt_predict_cv_async)
    def track_guess(self, slot1, slot2, fl, guess):
        """klt_track_guess on a copy: (records, number still tracked); `guess` a record array of the same length."""
        fl = np.ascontiguousarray(fl, FEAT_DTYPE).copy()
        guess = np.ascontiguousarray(guess, FEAT_DTYPE)
        if len(guess) != len(fl):
            raise ValueError("the guess list has %d records, the feature list %d" % (len(guess), len(fl)))
        k = C.c_int()
        self._check(self._lib.klt_track_guess(self._h, slot1, slot2, fl.ctypes.data, guess.ctypes.data, len(fl), C.byref(k)))
        return fl, k.value

    def track_guess_async(self, slot1, slot2, fb_in, fb_guess, fb_out, n):
        self._check(self._lib.klt_track_guess_async(self._h, slot1, slot2, fb_in, fb_guess, fb_out, n))

    def track_fb_guess_async(self, slot1, slot2, fb_in, fb_guess, fb_out, n, fb_back=-1):
        self._check(self._lib.klt_track_fb_guess_async(self._h, slot1, slot2, fb_in, fb_guess, fb_out, n, fb_back))

    def track_guess_batch_async(self, pairs, n):
        """pairs: [(slot1, slot2, fb_in, fb_guess, fb_out), ...] -- one launch for all of them; fb_guess -1: that pair has no guess."""
        cols = _columns(pairs, 5)
        self._check(self._lib.klt_track_guess_batch_async(self._h, cols[0], cols[1], cols[2], cols[3], cols[4], len(pairs), n))

    def predict_cv_async(self, fb_prev, fb_cur, fb_guess, n):
        """klt_predict_cv_async: constant-velocity guesses for the list fb_cur from the list before it, fb_prev"""
        self._check(self._lib.klt_predict_cv_async(self._h, fb_prev, fb_cur, fb_guess, n))

    # ------------------------------------------------ affine consistency check
    def set_affine_params(self, ap):
        key = bytes(ap)
        if key != getattr(self, "_affine_key", None):
            self._check(self._lib.klt_set_affine_params(self._h, C.byref(ap)))
            self._affine_key = key

    def affine_alloc(self, state, n):
        self._check(self._lib.klt_affine_alloc(self._h, state, n))

    def affine_copy(self, dst, src, n, with_templates=False):
        """Device-side snapshot of the per-feature affine state (klt_affine_copy_async); asynchronous."""
        self._check(self._lib.klt_affine_copy_async(self._h, dst, src, n, int(bool(with_templates))))

    def affine_free(self, state):
        if getattr(self, "_h", None):
            self._check(self._lib.klt_affine_free(self._h, state))

    def slot_free(self, slot):
        if getattr(self, "_h", None):
            self._check(self._lib.klt_slot_free(self._h, slot))

    # ids handed to the reference-shaped API objects (tracking contexts: 3 slots; feature lists: affine state) are recycled
    # when those objects die (weakref finalizers in selectGoodFeatures.py / trackFeatures.py)
    def take_slots(self, count=3):
        free = self.__dict__.setdefault("_free_slot_bases", [])
        if free:
            return free.pop()
        base = getattr(self, "_next_slot", 0)
        self._next_slot = base + count
        return base

    def release_slots(self, base, count=3):
        """Finalizer of a tracking context (any thread, any moment -- the garbage collector runs it): never waits for the lock."""
        self._when_free(self._release_slots, base, count)

    def _release_slots(self, base, count):
        try:
            for k in range(count):
                self.slot_free(base + k)
        except KltBackendError:
            return
        self.__dict__.setdefault("_free_slot_bases", []).append(base)

    def _when_free(self, fn, *args):
        """Run fn(*args) under the context's lock if nobody holds it (or this thread does); otherwise leave it for the next holder
        (`settle_deferred`).  A finalizer that WAITED here could deadlock two threads whose collectors each free an object of the
        other's context."""
        if self.lock.acquire(blocking=False):
            try:
                fn(*args)
            finally:
                self.lock.release()
        else:
            self._deferred.append((fn, args))

    def settle_deferred(self):
        """(lock held) the releases finalizers left behind while another thread was inside the context"""
        while self._deferred:
            try:
                fn, args = self._deferred.popleft()
            except IndexError:
                return
            fn(*args)

    def take_affine_state(self):
        free = self.__dict__.setdefault("_free_affine_states", [])
        if free:
            return free.pop()
        sid = getattr(self, "_next_affine_state", 0)
        self._next_affine_state = sid + 1
        return sid

    def release_affine_state(self, sid):
        self._when_free(self._release_affine_state, sid)

    def _release_affine_state(self, sid):
        try:
            self.affine_free(sid)
        except KltBackendError:
            return
        self.__dict__.setdefault("_free_affine_states", []).append(sid)

    def affine_download(self, state, n):
        out = np.empty(n, AFFINE_DTYPE)
        self._check(self._lib.klt_affine_download(self._h, state, out.ctypes.data, n))
        return out

    def track_affine(self, slot1, slot2, fl, state):
        fl = np.ascontiguousarray(fl, FEAT_DTYPE).copy()
        k = C.c_int()
        self._check(self._lib.klt_track_affine(self._h, slot1, slot2, fl.ctypes.data, len(fl), state, C.byref(k)))
        return fl, k.value

    def track_affine_async(self, slot1, slot2, fb_in, fb_out, n, state):
        self._check(self._lib.klt_track_affine_async(self._h, slot1, slot2, fb_in, fb_out, n, state))

    # -------------------------------------------------------------------- frames
    def upload(self, slot, img):
        """img: 2-D uint8 or float32 array (the reference's `np.array(pil.convert("F"))`)."""
        a = np.asarray(img)
        if a.ndim != 2:
            raise ValueError("expected a 2-D image")
        if a.dtype == np.uint8:
            a = np.ascontiguousarray(a)
            self._check(self._lib.klt_upload_u8(self._h, slot, a.ctypes.data, a.shape[1], a.shape[0], a.shape[1]))
        else:
            a = np.ascontiguousarray(a, np.float32)
            self._check(self._lib.klt_upload_f32(self._h, slot, a.ctypes.data, a.shape[1], a.shape[0], a.shape[1]))

    def pinned_array(self, shape, dtype=np.uint8):
        """numpy array backed by pinned host memory (valid until the context is closed)."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = C.c_void_p()
        self._check(self._lib.klt_host_alloc(self._h, nbytes, C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def upload_async(self, slot, img):
        """img: 2-D uint8 or float32 array from pinned_array(); enqueued on the copy stream, no host synchronisation."""
        if img.dtype not in (np.uint8, np.float32) or img.ndim != 2 or not img.flags["C_CONTIGUOUS"]:
            raise ValueError("upload_async takes a C-contiguous 2-D uint8 or float32 array in pinned memory")
        fn = self._lib.klt_upload_u8_async if img.dtype == np.uint8 else self._lib.klt_upload_f32_async
        self._check(fn(self._h, slot, img.ctypes.data, img.shape[1], img.shape[0], img.shape[1]))

    def device_alloc(self, nbytes):
        """Device memory owned by the context (an address as int); freed by device_free or with the context."""
        p = C.c_void_p()
        self._check(self._lib.klt_device_alloc(self._h, int(nbytes), C.byref(p)))
        return p.value

    def device_write(self, dev, arr):
        """Synchronous copy of a C-contiguous array to device address `dev`."""
        a = np.ascontiguousarray(arr)
        self._check(self._lib.klt_device_write(self._h, C.c_void_p(dev), a.ctypes.data, a.nbytes))

    def device_free(self, dev):
        self._check(self._lib.klt_device_free(self._h, C.c_void_p(dev)))

    def adopt_u8(self, slot, dev, ncols, nrows):
        """The slot's frame IS the u8 image at device address `dev` (contiguous rows): read in place, not copied (klt_slot_adopt_u8)."""
        self._check(self._lib.klt_slot_adopt_u8(self._h, slot, C.c_void_p(dev), ncols, nrows, ncols))

    def upload_wait(self):
        """Host waits until every upload_async issued so far has left its pinned source buffer."""
        self._check(self._lib.klt_upload_wait(self._h))

    def staging(self, shape, count=2, dtype=np.uint8):
        """`count` pinned staging buffers of `shape` (uint8, or float32 for colour / float frames), cached per context (pinned memory is
        never handed out twice)."""
        cache = self.__dict__.setdefault("_staging", {})
        key = (tuple(shape), count, np.dtype(dtype).char)
        if key not in cache:
            cache[key] = [self.pinned_array(shape, dtype) for _ in range(count)]
        return cache[key]

    def staging_forget(self, shape, count=2, dtype=np.uint8):
        """Drops a cached staging set without freeing it (somebody may still write to it); the next staging() allocates anew."""
        self.__dict__.setdefault("_staging", {}).pop((tuple(shape), count, np.dtype(dtype).char), None)

    def build_pyramids(self, slot, sync=True):
        fn = self._lib.klt_build_pyramids if sync else self._lib.klt_build_pyramids_async
        self._check(fn(self._h, slot))

    def build_pyramids_batch(self, slots, sync=False):
        arr = (C.c_int * len(slots))(*slots)
        self._check(self._lib.klt_build_pyramids_batch_async(self._h, arr, len(slots)))
        if sync:
            self.sync()

    def level0_path(self):
        """(KLT_L0_* code, merged) of the last build's last group of frames: which kernel built level 0, and whether the gradients of
        levels >= 1 went out as one launch (klt_level0_path; a diagnostic -- every path gives the same planes)"""
        merged = C.c_int()
        code = self._check(self._lib.klt_level0_path(self._h, C.byref(merged)))
        return code, bool(merged.value)

    def level0_lean(self):
        """True if the last build's last group of frames went out lean: level 0 as the compact smoothed image alone, its gradients left
        to the tracker (klt_level0_lean, KLT_OPT_L0_LAZY_GRAD; a diagnostic -- lean and full builds give the same results)"""
        lean = C.c_int()
        self._check(self._lib.klt_level0_lean(self._h, C.byref(lean)))
        return bool(lean.value)

    def level0_lean_form(self):
        """Which kernel that group's level-0 launch was: 0 not lean, 1 the banded lean form, 2 the wave form (klt_level0_lean_form,
        KLT_OPT_L0_LEAN_FORM; a diagnostic -- every form gives the same planes)"""
        form = C.c_int()
        self._check(self._lib.klt_level0_lean_form(self._h, C.byref(form)))
        return form.value

    def set_option(self, option, value):
        self._check(self._lib.klt_set_option(self._h, option, int(value)))

    def pyramids_valid(self, slot):
        """True while the slot's pyramids are built and match the current parameters."""
        return bool(self._check(self._lib.klt_slot_state(self._h, slot)) & 2)

    def frame_resident(self, slot):
        """True while the slot holds a frame (raw pixels on the device)."""
        return bool(self._check(self._lib.klt_slot_state(self._h, slot)) & 1)

    def device_memory(self):
        """(free, total) bytes of the context's device"""
        f, t = C.c_size_t(), C.c_size_t()
        self._check(self._lib.klt_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def slot_generation(self, slot):
        """Number of the build that filled the slot's pyramids (travels with swap_slots); 0 without valid pyramids."""
        g = C.c_uint64()
        self._check(self._lib.klt_slot_generation(self._h, slot, C.byref(g)))
        return g.value

    def swap_slots(self, a, b):
        self._check(self._lib.klt_swap_slots(self._h, a, b))

    def level_dims(self, slot, level):
        nc, nr = C.c_int(), C.c_int()
        self._check(self._lib.klt_level_dims(self._h, slot, level, C.byref(nc), C.byref(nr)))
        return nc.value, nr.value

    def download_level(self, slot, pyramid, level):
        nc, nr = self.level_dims(slot, level)
        out = np.empty((nr, nc), np.float32)
        self._check(self._lib.klt_download_f32(self._h, slot, pyramid, level, out.ctypes.data))
        return out

    # ------------------------------------------------------------------ features
    def featbuf_upload(self, fb, fl):
        fl = np.ascontiguousarray(fl, FEAT_DTYPE)
        self._check(self._lib.klt_featbuf_upload(self._h, fb, fl.ctypes.data, len(fl)))

    def featbuf_download(self, fb, n):
        out = np.empty(n, FEAT_DTYPE)
        self._check(self._lib.klt_featbuf_download(self._h, fb, out.ctypes.data, n))
        return out

    def featbuf_download_into(self, fb, out):
        """Download out.size records of feature buffer `fb` straight into the C-contiguous record array `out`."""
        if out.dtype != FEAT_DTYPE or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("featbuf_download_into takes a C-contiguous array of klt_feat records")
        self._check(self._lib.klt_featbuf_download(self._h, fb, out.ctypes.data, out.size))

    def featbuf_download_async(self, fb, out):
        """Enqueue the download of len(out) records of feature buffer `fb` into the PINNED record array `out` (pinned_array(..., FEAT_DTYPE));
        the records are there after download_wait().  The host does not wait for queued work (klt_featbuf_download_async)."""
        self._check(self._lib.klt_featbuf_download_async(self._h, fb, out.ctypes.data, len(out)))

    def download_wait(self):
        self._check(self._lib.klt_download_wait(self._h))

    def featbuf_alloc(self, fb, n):
        self._check(self._lib.klt_featbuf_alloc(self._h, fb, n))

    def featbuf_view(self, fb_view, fb_parent, offset, n):
        self._check(self._lib.klt_featbuf_view(self._h, fb_view, fb_parent, offset, n))

    def featbuf_devptr(self, fb):
        return self._lib.klt_featbuf_devptr(self._h, fb)

    # ----------------------------------------------------------------- selection
    def select(self, slot, n, mode=SELECTING_ALL, fl=None, use_pyramid=False):
        """Returns (structured feature array, number placed)."""
        if fl is None:
            fl = np.zeros(n, FEAT_DTYPE)
            fl["x"] = -1
            fl["y"] = -1
            fl["val"] = -1
        fl = np.array(fl, FEAT_DTYPE)          # always a copy: the caller's array is never modified
        placed = C.c_int()
        self._check(self._lib.klt_select(self._h, slot, mode, int(bool(use_pyramid)), fl.ctypes.data, len(fl), C.byref(placed)))
        return fl, placed.value

    def min_distance_walk(self, keys, ncols, nrows, mindist, overwrite_all, fl):
        """klt_min_distance_walk: the greedy minimum-distance walk over the candidate keys in the given order; returns (a copy of
        `fl` with its free slots filled, number placed)."""
        keys = np.ascontiguousarray(keys, np.uint64)
        fl = np.array(fl, FEAT_DTYPE)
        placed = C.c_int()
        self._check(self._lib.klt_min_distance_walk(self._h, keys.ctypes.data if keys.size else None, int(keys.size), int(ncols),
                                                    int(nrows), int(mindist), int(bool(overwrite_all)), fl.ctypes.data, len(fl),
                                                    C.byref(placed)))
        return fl, placed.value

    def host_records(self, n):
        """(in, out): two pinned arrays of n klt_feat records -- the host side of the reference-shaped API's lists (no staging copy
        inside the runtime, and the copies can be asynchronous).  Valid until the next call that uses them.  Views of ONE pair of
        pinned arrays that only ever grows (to twice what was asked for): a script that alternates between lists of two lengths keeps
        one mapping of the tracker's feature buffers (`_map_records`; a pair per length was remapped -- with a device-wide wait each
        time -- whenever the length changed: ADVICE r5)."""
        pair = self.__dict__.get("_host_records")
        if pair is None or len(pair[0]) < n:
            if pair is not None:
                mapped = self.__dict__.get("_mapped_records")
                if mapped is not None:                                 # the tracker's feature buffers are these arrays: unmap first
                    for fb in mapped[2:]:
                        self._check(self._lib.klt_featbuf_map_host(self._h, fb, None, 0))
                    self._mapped_records = None
                for a in pair:
                    self._check(self._lib.klt_host_free(self._h, C.c_void_p(a.ctypes.data)))
                self._host_records = None
            cap = max(256, n if pair is None else 2 * n)
            pair = self._host_records = (self.pinned_array((cap,), FEAT_DTYPE), self.pinned_array((cap,), FEAT_DTYPE))
        return pair[0][:n], pair[1][:n]

    def select_records(self, slot, n, mode=SELECTING_ALL, use_pyramid=False, fb=None):
        """klt_select for the host API without its spare round trips: SELECTING_ALL needs no list on the way in (every slot is
        written), REPLACING_SOME sends host_records(n)[0] (filled by the caller) without waiting for the copy; one download brings
        the records back into host_records(n)[1], which is returned."""
        self.select_enqueue(slot, n, mode, use_pyramid, fb)
        return self.select_complete(n, fb)

    def select_enqueue(self, slot, n, mode=SELECTING_ALL, use_pyramid=False, fb=None):
        """First half of select_records: everything up to the host's look at the outcome is enqueued (klt_select_begin_async) on the
        list in host_records(n)[0] (filled by the caller for REPLACING_SOME); the caller does its own host work, then calls
        select_complete.  With MAP_RECORDS (the default) the feature buffer IS that pinned array -- the kernels update it in place, no
        copy either way; otherwise the list goes up first."""
        if fb is None:
            fb = _FB_API_IN if MAP_RECORDS else _FB_API_SELECT
        if MAP_RECORDS and fb == _FB_API_IN:
            self._map_records(n, _FB_API_IN, _FB_API_OUT)
        elif mode == REPLACING_SOME:
            self._check(self._lib.klt_featbuf_upload_async(self._h, fb, self.host_records(n)[0].ctypes.data, n))
        self._check(self._lib.klt_select_begin_async(self._h, slot, mode, int(bool(use_pyramid)), fb, n))

    def select_complete(self, n, fb=None):
        """Second half: waits for the selection (klt_select_finish); the records are host_records(n)[0] itself when the buffer is
        mapped, else they come back into host_records(n)[1] with one download."""
        if fb is None:
            fb = _FB_API_IN if MAP_RECORDS else _FB_API_SELECT
        self._check(self._lib.klt_select_finish(self._h))
        if MAP_RECORDS and fb == _FB_API_IN:
            # klt_select_finish has waited for the parallel passes' last launch -- but the sorted serial walk (no candidates at all, an
            # exclusion square too large for the passes' LDS tile, KLT_OPT_SELECT_PARALLEL_NMS = 0) completes inside
            # klt_select_begin_async WITHOUT a host wait: the download that used to follow was that wait.  The records are only in the
            # mapped array once the stream is idle (found by tests/fuzz/fuzz_seeds_r05.sh: 1 of 15 000 sequence trials; the regression
            # test fails three times out of three without this line).
            self._check(self._lib.klt_sync(self._h))
            return self.host_records(n)[0]
        rout = self.host_records(n)[1]
        self._check(self._lib.klt_featbuf_download(self._h, fb, rout.ctypes.data, n))
        return rout

    def track_records(self, slot1, slot2, n, state=None, fb_in=_FB_API_IN, fb_out=_FB_API_OUT):
        """klt_track / klt_track_affine on host_records(n): [0] (filled by the caller) goes up without waiting for the copy, the
        tracked records come back in [1], which is returned."""
        self.track_enqueue(slot1, slot2, n, state, True, fb_in, fb_out)
        return self.track_complete(n, fb_out)

    def _map_records(self, n, fb_in, fb_out):
        """feature buffers fb_in / fb_out ARE host_records(n) (klt_featbuf_map_host): the tracker reads and writes them in place"""
        self.host_records(n)                                       # (grows the pair if it has to -- and unmaps it first)
        rin, rout = self._host_records
        key = (rin.ctypes.data, rout.ctypes.data, fb_in, fb_out)
        if self.__dict__.get("_mapped_records") != key:
            self._check(self._lib.klt_featbuf_map_host(self._h, fb_in, rin.ctypes.data, len(rin)))
            self._check(self._lib.klt_featbuf_map_host(self._h, fb_out, rout.ctypes.data, len(rout)))
            self._mapped_records = key

    def track_enqueue(self, slot1, slot2, n, state=None, upload=True, fb_in=_FB_API_IN, fb_out=_FB_API_OUT, fb_check=False, guess=None):
        """The tracker is enqueued on the list in host_records(n)[0]; nothing is waited for.  With MAP_RECORDS (the default) the two
        feature buffers are those pinned arrays themselves and no copy is enqueued; otherwise the list goes up first (`upload`; not
        again when the tracker is only repeated on other pyramids).  `guess`: a record array of predicted positions (motion prior,
        never with an affine state); it goes up with the list."""
        if MAP_RECORDS:
            self._map_records(n, fb_in, fb_out)
        elif upload:
            self._check(self._lib.klt_featbuf_upload_async(self._h, fb_in, self.host_records(n)[0].ctypes.data, n))
        if guess is not None and upload:
            self._check(self._lib.klt_featbuf_upload(self._h, _FB_API_GUESS, guess.ctypes.data, n))
        self.track_dispatch_async(slot1, slot2, fb_in, fb_out, n, state, fb_check, None if guess is None else _FB_API_GUESS, _FB_API_BACK)

    def track_dispatch_async(self, slot1, slot2, fb_in, fb_out, n, state=None, fb_check=False, fb_guess=None, fb_back=None):
        """The tracker entry point for (state, fb_check, fb_guess), enqueued: the motion prior's with guesses in `fb_guess`, the
        forward-backward check's with `fb_check` (or both in one), the affine check's with a `state` (params.py refuses the two others
        beside it), else the plain tracker.  `fb_back` (None: not passed): where the forward-backward check keeps its backward records."""
        back = () if fb_back is None else (fb_back,)
        if fb_guess is not None:
            if fb_check:
                self.track_fb_guess_async(slot1, slot2, fb_in, fb_guess, fb_out, n, *back)
            else:
                self.track_guess_async(slot1, slot2, fb_in, fb_guess, fb_out, n)
        elif fb_check:                       # stateless like the plain tracker: may be enqueued ahead and repeated
            self.track_fb_async(slot1, slot2, fb_in, fb_out, n, *back)
        elif state is None:
            self.track_async(slot1, slot2, fb_in, fb_out, n)
        else:
            self.track_affine_async(slot1, slot2, fb_in, fb_out, n, state)

    def track_mark(self):
        """Marks the main stream behind the tracker just enqueued: track_complete(marked=True) then waits for THAT point, and work
        enqueued after the mark (the scores of the replacement that follows) keeps running while the host moves the columns."""
        if MAP_RECORDS:
            self._check(self._lib.klt_download_mark_async(self._h))
            return True
        return False

    def track_complete(self, n, fb_out=_FB_API_OUT, marked=False):
        """The records of the LAST tracker enqueued into fb_out, in host_records(n)[1] (a wait for the stream -- or for the mark --
        when the buffers are mapped, one synchronous download otherwise)."""
        rout = self.host_records(n)[1]
        if MAP_RECORDS and marked:
            self._check(self._lib.klt_download_wait(self._h))
        elif MAP_RECORDS:
            self._check(self._lib.klt_sync(self._h))
        else:
            self._check(self._lib.klt_featbuf_download(self._h, fb_out, rout.ctypes.data, n))
        return rout

    def select_async(self, slot, mode, use_pyramid, fb, n):
        self._check(self._lib.klt_select_async(self._h, slot, mode, int(bool(use_pyramid)), fb, n))

    def select_begin(self, slot, mode, use_pyramid, fb, n):
        """First half of select_async: everything enqueued up to the host's look at the outcome (klt_select_begin_async)."""
        self._check(self._lib.klt_select_begin_async(self._h, slot, mode, int(bool(use_pyramid)), fb, n))

    def select_finish(self):
        """Second half: waits, and completes the selection (klt_select_finish).  True when the list was rewritten after the first half's
        launches had run: work enqueued in between that read the list (a tracker launch of the next frame) must be enqueued again."""
        return self._check(self._lib.klt_select_finish(self._h)) > 0

    def select_prepare(self, slot):
        """Scores of the slot's level-0 images ahead of a REPLACING_SOME selection on it (klt_select_prepare_async); asynchronous."""
        self._check(self._lib.klt_select_prepare_async(self._h, slot))

    # ------------------------------------------------------------- selection mask
    # `_mask_state`: what the host layer knows of the context's mask -- None: there is none; an array: the copy of the bytes
    # sync_select_mask sent; "direct": set by a caller of the two methods below (or a call that failed half way): unknown bytes
    def set_select_mask(self, mask):
        """klt_set_select_mask: `mask` a 2-D uint8 array (a byte of 0 = never a candidate; rows may be strided), copied to the device
        before this returns; None removes the mask.  What every later selection of this context honours, until it is set again."""
        self._mask_state = "direct"
        if mask is None:
            self._check(self._lib.klt_set_select_mask(self._h, None, 0, 0, 0))
            self._mask_state = None
            return
        a = np.asarray(mask)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError("set_select_mask takes a 2-D uint8 array")
        if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
            a = np.ascontiguousarray(a)
        self._check(self._lib.klt_set_select_mask(self._h, a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]))

    def set_select_mask_device(self, dev, ncols, nrows):
        """klt_set_select_mask_device: the mask IS the [nrows][ncols] bytes at device address `dev` (device_alloc / device_write, or
        another library's buffer; a multiple of 16), read in place by every selection; None removes the mask."""
        self._mask_state = "direct"
        self._check(self._lib.klt_set_select_mask_device(self._h, None if dev is None else C.c_void_p(dev), int(ncols), int(nrows)))
        if dev is None:
            self._mask_state = None

    def sync_select_mask(self, mask):
        """The reference-shaped API's mask (params.selection_mask_from_tc: None or a C-contiguous 2-D uint8 array): sent only when its
        bytes differ from the copy kept of what the context holds (klt_host_compare), so an array changed in place takes effect and
        an unchanged one costs one pass over it."""
        state = self.__dict__.get("_mask_state")
        if mask is None:
            if state is not None:
                self.set_select_mask(None)
            return
        from ._frames import same_pixels
        if isinstance(state, np.ndarray) and same_pixels(state, mask):
            return
        self.set_select_mask(mask)
        self._mask_state = mask.copy()

    # ------------------------------------------------------------- selection grid
    def set_select_grid(self, grid):
        """klt_set_select_grid: `grid` = (cell_width, cell_height, max_per_cell), or None for no grid.  No cell of cell_width x cell_height
        pixels holds more than max_per_cell features after a selection of this context, until it is set again."""
        self._grid_state = "direct"
        if grid is None:
            self._check(self._lib.klt_set_select_grid(self._h, None))
            self._grid_state = None
            return
        cw, ch, q = grid
        g = KltSelectGrid(int(cw), int(ch), int(q))
        self._check(self._lib.klt_set_select_grid(self._h, C.byref(g)))
        self._grid_state = (int(cw), int(ch), int(q))

    def select_grid_path(self):
        """klt_select_grid_path: 0 no selection under a grid yet, 1 filter kernel before the rank placement, 2 quota inside the walk"""
        return self._check(self._lib.klt_select_grid_path(self._h))

    def sync_select_grid(self, grid):
        """The reference-shaped API's grid (params.select_grid_from_tc: None or a tuple of three ints): sent only when it differs from
        what the context holds."""
        if self.__dict__.get("_grid_state") != grid:
            self.set_select_grid(grid)

    def select_intermediate(self, what):
        nc, nr = C.c_int(), C.c_int()
        self._check(self._lib.klt_select_dims(self._h, what, C.byref(nc), C.byref(nr)))
        out = np.empty((nr.value, nc.value), np.float32)
        self._check(self._lib.klt_download_select_f32(self._h, what, out.ctypes.data))
        return out

    def set_score_override(self, val):
        """Test hook: the next selection uses this [ny][nx] eigenvalue map instead of computing one."""
        val = np.ascontiguousarray(val, np.float32)
        self._check(self._lib.klt_set_score_override(self._h, val.ctypes.data, val.size))

    def prepared_keys(self, slot):
        """The [ny][nx] uint64 keys (scan order; f32 bits of val << 32 | x << 16 | y, 0 = below the threshold) of the score set that
        select_prepare computed for the slot's current contents (klt_download_prepared_keys; a diagnostic -- the set is not consumed)."""
        cap = 1 << 16
        while True:
            out = np.empty(cap, np.uint64)
            nx, ny = C.c_int(), C.c_int()
            rc = self._lib.klt_download_prepared_keys(self._h, slot, out.ctypes.data, cap, C.byref(nx), C.byref(ny))
            if rc == -1 and nx.value * ny.value > cap:           # KLT_ERR_ARG: the grid is larger than the buffer, and now known
                cap = nx.value * ny.value
                continue
            self._check(rc)
            return out[:nx.value * ny.value].reshape(ny.value, nx.value).copy()

    def select_score_path(self):
        """(rows, cols): which kernels built the summed-area tables of the last preparation or selection (klt_select_score_path) --
        rows 0 barrier / 1 pipeline; cols 0 barrier / 1 pipeline / 2 fused with the eigenvalue keys.  A diagnostic: every path gives
        the same tables."""
        rows, cols = C.c_int(), C.c_int()
        self._check(self._lib.klt_select_score_path(self._h, C.byref(rows), C.byref(cols)))
        return rows.value, cols.value

    def select_pick_path(self):
        """klt_select_pick_path: how the last completed selection got from the keys to the list, as a dict -- walk 0 serial / 1 parallel;
        order 0 greedy walk only / 1 ranked by counting / 2 accepted keys sorted and walked; cut 0 / 1 prefilter planned; attempts 1 / 2;
        passes launched; host looks; instantiation 9 / 0; pass_lds bytes; grid 0 LDS / 1 global; sparse 0 / 1.  A diagnostic: every path
        gives the same list."""
        from ._abi import KltSelectPick
        p = KltSelectPick()
        self._check(self._lib.klt_select_pick_path(self._h, C.byref(p)))
        return {k: int(getattr(p, k)) for k, _ in KltSelectPick._fields_}

    def sorted_candidates(self, n):
        val = np.empty(n, np.float32)
        x = np.empty(n, np.int32)
        y = np.empty(n, np.int32)
        nv = C.c_int()
        self._check(self._lib.klt_download_sorted_candidates(self._h, val.ctypes.data, x.ctypes.data, y.ctypes.data, n, C.byref(nv)))
        return val[:nv.value], x[:nv.value], y[:nv.value]

    # ------------------------------------------------------------------ tracking
    def track(self, slot1, slot2, fl):
        """In-place on a copy: returns (structured feature array, number still tracked)."""
        fl = np.ascontiguousarray(fl, FEAT_DTYPE).copy()
        k = C.c_int()
        self._check(self._lib.klt_track(self._h, slot1, slot2, fl.ctypes.data, len(fl), C.byref(k)))
        return fl, k.value

    def track_async(self, slot1, slot2, fb_in, fb_out, n):
        self._check(self._lib.klt_track_async(self._h, slot1, slot2, fb_in, fb_out, n))

    def track_batch_async(self, pairs, n):
        """pairs: [(slot1, slot2, fb_in, fb_out), ...] -- one tracker launch for all of them."""
        cols = _columns(pairs, 4)
        self._check(self._lib.klt_track_batch_async(self._h, cols[0], cols[1], cols[2], cols[3], len(pairs), n))

    # ------------------------------------------------ per-feature track quality (klt_track_quality*)
    def track_quality(self, slot1, slot2, fl_in, fl_out):
        """klt_track_quality: a QUALITY_DTYPE array (residue, ncc, min_eig, val), record i measured between fl_in[i] on slot1's level 0 and
        fl_out[i] on slot2's; val 1 = measured, else the record is all zero."""
        fl_in = np.ascontiguousarray(fl_in, FEAT_DTYPE)
        fl_out = np.ascontiguousarray(fl_out, FEAT_DTYPE)
        if len(fl_in) != len(fl_out):
            raise ValueError("the two lists have %d and %d records" % (len(fl_in), len(fl_out)))
        q = np.zeros(len(fl_in), QUALITY_DTYPE)
        self._check(self._lib.klt_track_quality(self._h, slot1, slot2, fl_in.ctypes.data, fl_out.ctypes.data, q.ctypes.data, len(fl_in)))
        return q

    def track_quality_async(self, slot1, slot2, fb_in, fb_out, fb_quality, n):
        self._check(self._lib.klt_track_quality_async(self._h, slot1, slot2, fb_in, fb_out, fb_quality, n))

    def track_quality_batch_async(self, pairs, n):
        """pairs: [(slot1, slot2, fb_in, fb_out, fb_quality), ...] -- one quality launch for all of them."""
        cols = _columns(pairs, 5)
        self._check(self._lib.klt_track_quality_batch_async(self._h, cols[0], cols[1], cols[2], cols[3], cols[4], len(pairs), n))

    def quality_download(self, fb, n):
        """n quality records of feature buffer `fb` (what a track_quality*_async launch wrote there)"""
        return self.featbuf_download(fb, n).view(QUALITY_DTYPE)

    # ------------------------------------------------ descriptors and their matcher (klt_describe*, klt_match*)
    def set_descriptor_params(self, mode=1):
        """klt_set_descriptor_params: 1 upright (the default), 2 steered by the patch's orientation"""
        self._check(self._lib.klt_set_descriptor_params(self._h, C.byref(KltDescriptorParams(int(mode)))))

    def describe_async(self, slot, fb_in, fb_desc, n):
        self._check(self._lib.klt_describe_async(self._h, slot, fb_in, fb_desc, n))

    def describe(self, slot, fl, sync_entry=False):
        """A DESCRIPTOR_DTYPE array, record i the descriptor of fl[i] on the 8-bit frame the slot holds (behind its ingest stages).
        sync_entry: through klt_describe and the library's staging buffers instead of the Python layer's own two."""
        fl = np.ascontiguousarray(fl, FEAT_DTYPE)
        n = len(fl)
        if sync_entry:
            out = np.zeros(n, DESCRIPTOR_DTYPE)
            self._check(self._lib.klt_describe(self._h, slot, fl.ctypes.data, out.ctypes.data, n))
            return out
        if n:
            self.featbuf_upload(_FB_API_DESCRIBE_IN, fl)
        self.describe_async(slot, _FB_API_DESCRIBE_IN, _FB_API_DESCRIBE, n)
        return self.descriptor_download(_FB_API_DESCRIBE, n)

    def descriptor_upload(self, fb, desc):
        desc = np.ascontiguousarray(desc, DESCRIPTOR_DTYPE)
        self.featbuf_upload(fb, desc.view(FEAT_DTYPE))

    def descriptor_download(self, fb, n):
        """n descriptors of feature buffer `fb` (its first 3 n records)"""
        if n == 0:
            return np.zeros(0, DESCRIPTOR_DTYPE)
        return self.featbuf_download(fb, 3 * n).view(DESCRIPTOR_DTYPE)

    def set_match_params(self, max_distance=64, ratio_num=4, ratio_den=5, cross_check=1, radius=0):
        """klt_set_match_params (the defaults are the library's)"""
        p = KltMatchParams(int(max_distance), int(ratio_num), int(ratio_den), int(cross_check), int(radius))
        self._check(self._lib.klt_set_match_params(self._h, C.byref(p)))

    def match_async(self, fb_query, nq, fb_train, nt, fb_match):
        self._check(self._lib.klt_match_async(self._h, fb_query, nq, fb_train, nt, fb_match))

    def match(self, query, train, sync_entry=False):
        """A MATCH_DTYPE array, one record per query descriptor, under the parameters the context holds (set_match_params)"""
        query = np.ascontiguousarray(query, DESCRIPTOR_DTYPE)
        train = np.ascontiguousarray(train, DESCRIPTOR_DTYPE)
        nq, nt = len(query), len(train)
        if sync_entry:
            out = np.zeros(nq, MATCH_DTYPE)
            self._check(self._lib.klt_match(self._h, query.ctypes.data, nq, train.ctypes.data, nt, out.ctypes.data))
            return out
        if nq == 0:
            return np.zeros(0, MATCH_DTYPE)
        self.descriptor_upload(_FB_API_MATCH_QUERY, query)
        if nt:
            self.descriptor_upload(_FB_API_MATCH_TRAIN, train)
        self.match_async(_FB_API_MATCH_QUERY, nq, _FB_API_MATCH_TRAIN, nt, _FB_API_MATCH)
        return self.featbuf_download(_FB_API_MATCH, nq).view(MATCH_DTYPE)

    def match_path(self):
        """klt_match_path: how many ranges the train set of the last match was cut into"""
        splits = C.c_int(0)
        self._check(self._lib.klt_match_path(self._h, C.byref(splits)))
        return splits.value

    # ------------------------------------------------ track identities (klt_reacquire_*)
    def set_reacquire_params(self, capacity=1024, max_gap=30, max_distance=64, ratio_num=4, ratio_den=5, radius=24):
        """klt_set_reacquire_params (the defaults are the library's); ends the sequence in progress"""
        p = KltReacquireParams(int(capacity), int(max_gap), int(max_distance), int(ratio_num), int(ratio_den), int(radius))
        self._check(self._lib.klt_set_reacquire_params(self._h, C.byref(p)))

    def reacquire_begin_async(self, slot, fb_list, fb_ident, n):
        self._check(self._lib.klt_reacquire_begin_async(self._h, slot, fb_list, fb_ident, n))

    def reacquire_step_async(self, slot, fb_list, fb_ident_prev, fb_ident, n):
        self._check(self._lib.klt_reacquire_step_async(self._h, slot, fb_list, fb_ident_prev, fb_ident, n))

    def ident_download(self, fb, n):
        """n ident records of feature buffer `fb`"""
        return self.featbuf_download(fb, n).view(IDENT_DTYPE)

    def reacquire_state(self):
        """klt_reacquire_state (synchronous): a REACQUIRE_STATE_DTYPE scalar -- k, h, next_id, the valid bank entries, the fresh and the
        deposited slots of the last step"""
        st = KltReacquireState()
        self._check(self._lib.klt_reacquire_state(self._h, C.byref(st)))
        out = np.zeros((), REACQUIRE_STATE_DTYPE)
        for k in REACQUIRE_STATE_DTYPE.names:
            out[k] = getattr(st, k)
        return out

    def reacquire_bank(self, capacity):
        """klt_reacquire_download_bank (synchronous): the `capacity` entries of the bank as a BANK_DTYPE array"""
        out = np.zeros(int(capacity), BANK_DTYPE)
        self._check(self._lib.klt_reacquire_download_bank(self._h, out.ctypes.data))
        return out

    def reacquire_path(self):
        """klt_reacquire_path: the launches the last begin (2) or step (5) enqueued; 0: none yet"""
        launches = C.c_int(-1)
        self._check(self._lib.klt_reacquire_path(self._h, C.byref(launches)))
        return launches.value

    # ------------------------------------------------ the post-track stages (params.post_track_from_tc): one chain
    def set_post_track_params(self, stages):
        """the parameters of every stage that is switched on, once for a call that enqueues the chain many times (KLTTrackSequence)"""
        for k, p in stages.consensus:
            self._consensus_set_params(k, p, {})
        if stages.crowd is not None:
            self.set_crowd_params(stages.crowd)

    def post_track_async(self, stages, slot1, slot2, fb_in, fb_out, n, targets, set_params=False, ages=None):
        """What follows a tracker launch from fb_in into fb_out, enqueued in THE order: the consensus check that is switched on -- it
        rewrites fb_out in place --, then the crowding check on fb_out, then the quality launch: a record that either check flagged is
        simply unmeasured.  A repeated tracker is followed by the whole chain again.  `targets` (PostTrackTargets, or anything with its
        attributes: each is read when its stage is enqueued, and only then) names the buffers written: model (None: the check's own
        buffer of a KLTTrackFeatures call), crowd_prev (the crowd records of the step before, -1: none), crowd, quality.  `set_params`:
        each stage's parameters are set directly in front of its launch (KLTTrackFeatures: one or two chains per call); `ages`: crowd
        records that go up into targets.crowd_prev first."""
        for k, p in stages.consensus:
            if set_params:
                self._consensus_set_params(k, p, {})
            fb_model = targets.model
            self._consensus_async(k, fb_in, fb_out, k.fb_api if fb_model is None else fb_model, n)
        if stages.crowd is not None:
            if set_params:
                self.set_crowd_params(stages.crowd)
            fb_prev = targets.crowd_prev
            if ages is not None:
                self.featbuf_upload(fb_prev, ages)
            self.crowd_check_async(fb_out, fb_prev, targets.crowd, n)
        if stages.quality:
            self.track_quality_async(slot1, slot2, fb_in, fb_out, targets.quality, n)

    # ------------------------------------------------ the consensus checks (a row of CONSENSUS_CHECKS each): one implementation
    def _consensus_set_params(self, k, p, kw):
        if p is None:
            d = dict(k.defaults, mode=1)
            d.update(kw)
            p = k.params_type(**d)
        key = bytes(p)
        if key != self._consensus_keys.get(k.name):          # (cached by bytes: the same parameters again cost no call)
            self._consensus_keys.pop(k.name, None)
            self._check(getattr(self._lib, "klt_set_%s_params" % k.name)(self._h, C.byref(p)))
            self._consensus_keys[k.name] = key

    def _consensus_check(self, k, fl_in, fl_out):
        fl_in = np.ascontiguousarray(fl_in, FEAT_DTYPE)
        out = np.array(fl_out, FEAT_DTYPE, order="C")
        if len(fl_in) != len(out):
            raise ValueError("the two lists have %d and %d records" % (len(fl_in), len(out)))
        model = np.zeros(1, k.dtype)
        cnt = C.c_int(0)
        self._check(getattr(self._lib, "klt_%s_check" % k.c_check)(self._h, fl_in.ctypes.data, out.ctypes.data,
                                                                   C.cast(model.ctypes.data, C.POINTER(k.model_type)), len(out), C.byref(cnt)))
        return out, model[0], cnt.value

    def _consensus_async(self, k, fb_in, fb_out, fb_model, n):
        self._check(getattr(self._lib, "klt_%s_check_async" % k.c_check)(self._h, fb_in, fb_out, fb_model, n))

    def _consensus_batch_async(self, k, pairs, n):
        cols = _columns(pairs, 3)
        self._check(getattr(self._lib, "klt_%s_check_batch_async" % k.c_check)(self._h, cols[0], cols[1], cols[2], len(pairs), n))

    def _consensus_path(self, k):
        return self._check(getattr(self._lib, "klt_%s_check_path" % k.c_check)(self._h))

    def _consensus_download(self, k, fb):
        return self.featbuf_download(fb, k.records).view(k.dtype)[0]

    # ------------------------------------------------ motion-model check (klt_set_model_params, klt_motion_check*)
    def set_model_params(self, mp=None, **kw):
        """klt_set_model_params: `mp` a KltModelParams, or its fields by name (mode, ncols, nrows, hypotheses, seed, min_inliers,
        max_error, min_area; defaults 1, -, -, 256, 0, 8, 1.0, 1.0)"""
        self._consensus_set_params(_MODEL_CHECK, mp, kw)

    def motion_check(self, fl_in, fl_out):
        """klt_motion_check: (out, model, n_outliers) -- fl_out with every tracked record off the dominant affine motion turned into
        (-1, -1, KLT_MODEL_OUTLIER, aux), the MODEL_DTYPE record, and how many records that were"""
        return self._consensus_check(_MODEL_CHECK, fl_in, fl_out)

    def motion_check_async(self, fb_in, fb_out, fb_model, n):
        self._consensus_async(_MODEL_CHECK, fb_in, fb_out, fb_model, n)

    def motion_check_batch_async(self, pairs, n):
        """pairs: [(fb_in, fb_out, fb_model), ...] -- the check's launches once for all of them."""
        self._consensus_batch_async(_MODEL_CHECK, pairs, n)

    def motion_check_path(self):
        """klt_motion_check_path: 0 no motion-check launch yet, 1 the last one ran on one pair, 2 on a table of pairs (a diagnostic)"""
        return self._consensus_path(_MODEL_CHECK)

    def model_download(self, fb):
        """the MODEL_DTYPE record of feature buffer `fb` (what a motion_check*_async launch wrote there)"""
        return self._consensus_download(_MODEL_CHECK, fb)

    # ------------------------------------------------ epipolar check (klt_set_epipolar_params, klt_epipolar_check*)
    def set_epipolar_params(self, ep=None, **kw):
        """klt_set_epipolar_params: `ep` a KltEpipolarParams, or its fields by name (mode, ncols, nrows, hypotheses, seed, min_inliers,
        max_error; defaults 1, -, -, 512, 0, 16, 1.0)"""
        self._consensus_set_params(_EPIPOLAR_CHECK, ep, kw)

    def epipolar_check(self, fl_in, fl_out):
        """klt_epipolar_check: (out, model, n_outliers) -- fl_out with every tracked record off the pair's fundamental matrix turned into
        (-1, -1, KLT_EPIPOLAR_OUTLIER, aux), the EPIPOLAR_DTYPE record, and how many records that were"""
        return self._consensus_check(_EPIPOLAR_CHECK, fl_in, fl_out)

    def epipolar_check_async(self, fb_in, fb_out, fb_model, n):
        self._consensus_async(_EPIPOLAR_CHECK, fb_in, fb_out, fb_model, n)

    def epipolar_check_batch_async(self, pairs, n):
        """pairs: [(fb_in, fb_out, fb_model), ...] -- the check's launches once for all of them."""
        self._consensus_batch_async(_EPIPOLAR_CHECK, pairs, n)

    def epipolar_check_path(self):
        """klt_epipolar_check_path: 0 no epipolar-check launch yet, 1 the last one ran on one pair, 2 on a table of pairs (a diagnostic)"""
        return self._consensus_path(_EPIPOLAR_CHECK)

    def epipolar_download(self, fb):
        """the EPIPOLAR_DTYPE record of feature buffer `fb` (what an epipolar_check*_async launch wrote there)"""
        return self._consensus_download(_EPIPOLAR_CHECK, fb)

    # ------------------------------------------------ homography check (klt_set_homography_params, klt_homography_check*)
    def set_homography_params(self, hp=None, **kw):
        """klt_set_homography_params: `hp` a KltHomographyParams, or its fields by name (mode, ncols, nrows, hypotheses, seed, min_inliers,
        max_error; defaults 1, -, -, 256, 0, 8, 1.0)"""
        self._consensus_set_params(_HOMOGRAPHY_CHECK, hp, kw)

    def homography_check(self, fl_in, fl_out):
        """klt_homography_check: (out, model, n_outliers) -- fl_out with every tracked record off the pair's homography turned into
        (-1, -1, KLT_HOMOGRAPHY_OUTLIER, aux), the HOMOGRAPHY_DTYPE record, and how many records that were"""
        return self._consensus_check(_HOMOGRAPHY_CHECK, fl_in, fl_out)

    def homography_check_async(self, fb_in, fb_out, fb_model, n):
        self._consensus_async(_HOMOGRAPHY_CHECK, fb_in, fb_out, fb_model, n)

    def homography_check_batch_async(self, pairs, n):
        """pairs: [(fb_in, fb_out, fb_model), ...] -- the check's launches once for all of them."""
        self._consensus_batch_async(_HOMOGRAPHY_CHECK, pairs, n)

    def homography_check_path(self):
        """klt_homography_check_path: 0 no homography-check launch yet, 1 the last one ran on one pair, 2 on a table of pairs (a diagnostic)"""
        return self._consensus_path(_HOMOGRAPHY_CHECK)

    def homography_download(self, fb):
        """the HOMOGRAPHY_DTYPE record of feature buffer `fb` (what a homography_check*_async launch wrote there)"""
        return self._consensus_download(_HOMOGRAPHY_CHECK, fb)

    # ------------------------------------------------ crowding check (klt_set_crowd_params, klt_crowd_check*)
    def set_crowd_params(self, cp=None, **kw):
        """klt_set_crowd_params: `cp` a KltCrowdParams, or its fields by name (mode, ncols, nrows, min_distance; defaults 1, -, -, 1)"""
        if cp is None:
            d = dict(mode=1, min_distance=1)
            d.update(kw)
            cp = KltCrowdParams(**d)
        key = bytes(cp)
        if key != getattr(self, "_crowd_key", None):
            self._crowd_key = None
            self._check(self._lib.klt_set_crowd_params(self._h, C.byref(cp)))
            self._crowd_key = key

    def crowd_check(self, fl_out, prev=None):
        """klt_crowd_check: (out, crowd, n_crowded) -- fl_out with every tracked record that lies within min_distance of an older one
        turned into (-1, -1, KLT_CROWDED, aux), the CROWD_DTYPE records, and how many records that were.  `prev`: the CROWD_DTYPE
        records of the previous step (their age column counts), or None."""
        out = np.array(fl_out, FEAT_DTYPE, order="C")
        if prev is not None:
            prev = np.ascontiguousarray(prev, CROWD_DTYPE)
            if len(prev) != len(out):
                raise ValueError("the list has %d records, prev %d" % (len(out), len(prev)))
        crowd = np.zeros(len(out), CROWD_DTYPE)
        cnt = C.c_int(0)
        self._check(self._lib.klt_crowd_check(self._h, out.ctypes.data, prev.ctypes.data if prev is not None else None, crowd.ctypes.data,
                                              len(out), C.byref(cnt)))
        return out, crowd, cnt.value

    def crowd_check_async(self, fb_out, fb_prev, fb_crowd, n):
        """fb_prev: -1 or None = no previous step"""
        self._check(self._lib.klt_crowd_check_async(self._h, fb_out, -1 if fb_prev is None else fb_prev, fb_crowd, n))

    def crowd_check_batch_async(self, lists, n):
        """lists: [(fb_out, fb_prev, fb_crowd), ...] (fb_prev -1: none) -- the check's launches once for all of them."""
        cols = _columns(lists, 3)
        self._check(self._lib.klt_crowd_check_batch_async(self._h, cols[0], cols[1], cols[2], len(lists), n))

    def crowd_check_path(self):
        """klt_crowd_check_path: 0 no crowd-check launch yet, 1 the last one ran on one list, 2 on a table of lists (a diagnostic)"""
        return self._check(self._lib.klt_crowd_check_path(self._h))

    def crowd_check_rounds(self, phases=False):
        """klt_crowd_check_rounds: the rounds the last launch's (first) list took; waits for it (a diagnostic).  `phases`: (rounds,
        (grouping, rounds, records) in us) -- what the resolve launch's workgroup spent where"""
        r = C.c_int(0)
        ticks = (C.c_int * 3)()
        self._check(self._lib.klt_crowd_check_rounds(self._h, C.byref(r), ticks))
        return (r.value, tuple(t * 0.01 for t in ticks)) if phases else r.value

    def crowd_download(self, fb, n):
        """n crowd records of feature buffer `fb` (what a crowd_check*_async launch wrote there)"""
        return self.featbuf_download(fb, n).view(CROWD_DTYPE)

    def track_stats_reset(self):
        self._check(self._lib.klt_track_stats_reset(self._h))

    def track_stats(self):
        s = KltTrackStats()
        self._check(self._lib.klt_track_stats_read(self._h, C.byref(s)))
        return {"features": int(s.features),
                "level_visits": [int(v) for v in s.level_visits],
                "iterations": [int(v) for v in s.iterations]}

    # ------------------------------------------------------- multi-GPU (RCCL inside libkltgpu)
    def comm_init(self, nranks, rank, unique_id):
        """unique_id: the 128 bytes rank 0 got from klt_comm_unique_id (parallel.init_communicators exchanges them)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.klt_comm_init_rank(self._h, int(nranks), int(rank), buf))

    def comm_destroy(self):
        self._check(self._lib.klt_comm_destroy(self._h))

    def comm_info(self):
        n, r = C.c_int(), C.c_int()
        self._check(self._lib.klt_comm_info(self._h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def allgather_featbuf_async(self, fb_src, fb_dst, n):
        self._check(self._lib.klt_allgather_featbuf_async(self._h, fb_src, fb_dst, n))

    def gather_featbuf_async(self, fb_src, fb_dst, n, root=0):
        self._check(self._lib.klt_gather_featbuf_async(self._h, fb_src, fb_dst, n, root))

    def gatherv_featbuf_async(self, fb_src, fb_dst, counts, root=0):
        """Gather with a count per rank (shards of unequal size): rank r contributes counts[r] records (klt_gatherv_featbuf_async)."""
        arr = (C.c_int * len(counts))(*[int(v) for v in counts])
        self._check(self._lib.klt_gatherv_featbuf_async(self._h, fb_src, fb_dst, arr, root))

    def comm_set_timeout(self, ms):
        """Host-side waits on the communicator give up after `ms` milliseconds (KLT_ERR_TIMEOUT) instead of hanging."""
        self._check(self._lib.klt_comm_set_timeout(self._h, float(ms)))

    def sendrecv_featbuf(self, fb_send, to, fb_recv, frm, n):
        """The feature list as a baton (klt_sendrecv_featbuf_async): n records of fb_send to rank `to` and / or from rank `frm` into
        fb_recv (-1: no such side); the context's stream waits for the arrival."""
        self._check(self._lib.klt_sendrecv_featbuf_async(self._h, fb_send, to, fb_recv, frm, n))

    def comm_fence(self):
        """The context's stream waits (on the device) for the collectives issued so far."""
        self._check(self._lib.klt_comm_fence_async(self._h))

    def comm_fence_featbuf(self, fb):
        """... only for the last collective that read or wrote feature buffer `fb`."""
        self._check(self._lib.klt_comm_fence_featbuf_async(self._h, fb))

    def comm_wait(self):
        self._check(self._lib.klt_comm_wait(self._h))

    def comm_allreduce_max(self, values):
        """Element-wise max over all ranks of up to 16 floats; synchronous (doubles as a barrier)."""
        a = (C.c_double * len(values))(*values)
        self._check(self._lib.klt_comm_allreduce_max(self._h, a, len(values)))
        return list(a)

    # -------------------------------------------------- standalone convolutions
    def convolve_separate(self, img, horiz, vert):
        """_convolveSeparate (klt_convolve_separate_f32): any two tap lists"""
        img = np.ascontiguousarray(img, np.float32)
        out = np.empty_like(img)
        self._check(self._lib.klt_convolve_separate_f32(self._h, img.ctypes.data, img.shape[1], img.shape[0], _dp(horiz), len(horiz),
                                                        _dp(vert), len(vert), out.ctypes.data))
        return out

    def smooth(self, img, gauss):
        img = np.ascontiguousarray(img, np.float32)
        out = np.empty_like(img)
        self._check(self._lib.klt_smooth_f32(self._h, img.ctypes.data, img.shape[1], img.shape[0], _dp(gauss), len(gauss),
                                             out.ctypes.data))
        return out

    def pyramid(self, img, subsampling, nlevels, gauss):
        """[level 1, ..., level nlevels-1] of KLTPyramid.Compute (klt_pyramid_f32): every level smoothed and subsampled on the device."""
        img = np.ascontiguousarray(img, np.float32)
        dims, (nr, nc) = [], img.shape
        for _ in range(1, nlevels):
            nc, nr = nc // subsampling, nr // subsampling
            dims.append((nr, nc))
        out = np.empty(sum(r * c for r, c in dims), np.float32)
        self._check(self._lib.klt_pyramid_f32(self._h, img.ctypes.data, img.shape[1], img.shape[0], nlevels, subsampling, _dp(gauss), len(gauss),
                                              out.ctypes.data))
        levels, off = [], 0
        for r, c in dims:
            levels.append(out[off:off + r * c].reshape(r, c))
            off += r * c
        return levels

    def gradients(self, img, gauss, deriv):
        img = np.ascontiguousarray(img, np.float32)
        gx = np.empty_like(img)
        gy = np.empty_like(img)
        self._check(self._lib.klt_gradients_f32(self._h, img.ctypes.data, img.shape[1], img.shape[0], _dp(gauss), len(gauss),
                                                _dp(deriv), len(deriv), gx.ctypes.data, gy.ctypes.data))
        return gx, gy

    # -------------------------------------------------------------------- timing
    def timing_enable(self, on=True):
        """1 / True: an event pair around every launch; 2: the level-0 pyramid launch by its dispatch's own timestamps (klt_gpu.h)."""
        self._check(self._lib.klt_timing_enable(self._h, int(on)))

    def timing_read(self):
        buf = (KltKernelTime * 32)()
        n = self._check(self._lib.klt_timing_read(self._h, buf, 32))
        return [{"name": buf[i].name.decode(), "launches": int(buf[i].launches), "total_ms": float(buf[i].total_ms),
                 "bytes": float(buf[i].bytes)} for i in range(n)]


_tls = threading.local()


def default_context(device=None):
    """The calling THREAD's context for `device` (created on first use): the one the reference-shaped Python API works on.

    One context per host thread and device (include/klt_gpu.h, "Threads"; SURVEY section 8(b): no shared mutable globals): two
    threads that each track their own video run on their own HIP streams, parameters and pinned record buffers, side by side.
    A tracking context (`KLT_TrackingContext`) stays with the context of the thread that first used it (`context_of`), because its
    frames and pyramids live in that context's slots; every KLT* call holds that context's lock, so a tracking context handed to
    another thread -- or shared by two -- is served one call at a time."""
    import os
    if device is None:
        device = int(os.environ.get("KLT_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        n = load_library().klt_device_count()
        if n > 0:
            device %= n
    table = _tls.__dict__.setdefault("contexts", {})
    ctx = table.get(device)
    if ctx is None or ctx._h is None:
        ctx = table[device] = Context(device)
    return ctx


def context_of(tc, device=None):
    """The context a tracking context is bound to: the calling thread's default context when `tc` is first used, the same one ever
    after (whichever thread calls)."""
    ctx = tc.__dict__.get("_klt_ctx")
    if ctx is None or ctx._h is None:
        ctx = tc.__dict__["_klt_ctx"] = default_context(device)
        tc.__dict__.pop("_klt_slots", None)                 # (slots of a context that was closed under it)
        tc.__dict__.pop("_klt_frames", None)
    return ctx


def model_affine(model):
    """klt_motion_model_affine: (A, t) of the map q = A p + t in uncentred pixel coordinates -- A a 2x2 float64 array, t of length 2 --
    from a MODEL_DTYPE record; (None, None) for one without a model (valid == 0)"""
    rec = np.zeros(1, MODEL_DTYPE)
    rec[0] = model
    A, t = np.zeros(4, np.float64), np.zeros(2, np.float64)
    dp = C.POINTER(C.c_double)
    rc = load_library().klt_motion_model_affine(C.cast(rec.ctypes.data, C.POINTER(KltMotionModel)), A.ctypes.data_as(dp), t.ctypes.data_as(dp))
    if rc != 0:
        return None, None
    return A.reshape(2, 2), t


def epipolar_matrix(model):
    """klt_epipolar_matrix: the 3x3 fundamental matrix F of an EPIPOLAR_DTYPE record in uncentred pixel coordinates, unit Frobenius norm,
    q^T F p = 0 for p in frame 1 and q in frame 2; None for a record without a model (valid == 0)"""
    rec = np.zeros(1, EPIPOLAR_DTYPE)
    rec[0] = model
    F = np.zeros(9, np.float64)
    rc = load_library().klt_epipolar_matrix(C.cast(rec.ctypes.data, C.POINTER(KltEpipolarModel)), F.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        return None
    return F.reshape(3, 3)


def homography_matrix(model):
    """klt_homography_matrix: the 3x3 homography H of a HOMOGRAPHY_DTYPE record in uncentred pixel coordinates, unit Frobenius norm,
    q ~ H p for p in frame 1 and q in frame 2, third coordinate positive at the image centre; None for a record without a model"""
    rec = np.zeros(1, HOMOGRAPHY_DTYPE)
    rec[0] = model
    H = np.zeros(9, np.float64)
    rc = load_library().klt_homography_matrix(C.cast(rec.ctypes.data, C.POINTER(KltHomographyModel)), H.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        return None
    return H.reshape(3, 3)


def model_summary(model):
    """what KLTTrackFeatures leaves in tc.model_last: a dict with A (2x2), t, valid, candidates, inliers, hypothesis"""
    A, t = model_affine(model)
    return {"A": A, "t": t, "valid": int(model["valid"]), "candidates": int(model["n_candidates"]), "inliers": int(model["n_inliers"]),
            "hypothesis": int(model["hypothesis"])}


__all__ = ["Context", "default_context", "context_of", "FEAT_DTYPE", "QUALITY_DTYPE", "MODEL_DTYPE", "model_affine", "model_summary", "EPIPOLAR_DTYPE", "epipolar_matrix", "HOMOGRAPHY_DTYPE", "homography_matrix", "CROWD_DTYPE", "SELECTING_ALL", "REPLACING_SOME", "KltBackendError", "KltCommTimeout", "KltOutOfMemory",
           "KLT_MAX_LEVELS", "KltParams"]
