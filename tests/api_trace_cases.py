"""Call traces of the Python API layer without a device: what KLTTrackSequence's host logic asks of a context, and what KLTTrackFeatures
asks of the library, call by call with normalised arguments.  tests/golden/gen_api_call_traces.py records them into
tests/golden/api_call_traces.json; tests/test_api_call_traces.py replays the same cases and wants the same traces.

sequence_trace    `_track_sequence_locked` on a stand-in for the context that logs every method call
features_trace    three `KLTTrackFeatures` calls on a real `Context` whose `_lib` is a stand-in that logs every klt_* call
"""
import ctypes as C
import hashlib
import itertools
import threading

import numpy as np

H, W = 48, 64

# name -> attributes of the tracking context
STAGE_OPTIONS = (
    ("none", {}),
    ("quality", dict(trackQuality=True)),
    ("model", dict(motionModelCheck="affine")),
    ("epipolar", dict(epipolarCheck=True)),
    ("homography", dict(homographyCheck=True)),
    ("crowd", dict(crowdingCheck=True)),
    ("fb", dict(forwardBackwardCheck=True)),
    ("predict", dict(motionPrediction="constant_velocity")),
    ("all", dict(forwardBackwardCheck=True, motionPrediction="constant_velocity", trackQuality=True, crowdingCheck=True, homographyCheck=True)),
    ("affine", dict(affineConsistencyCheck=2)),
    ("affine_quality", dict(affineConsistencyCheck=2, trackQuality=True)),
)
FRAME_COUNTS = (1, 2, 3, 4, 6, 70)                 # seventy frames cross the 64-row chunk of the record tables
FULL_TRACE_UP_TO = 6                                # longer sequences are kept as (entries, sha256)
ARRANGEMENTS = ((True, True, True), (True, False, True), (False, True, True), (True, True, False), (False, True, False))      # (replace_lost, async_ingest, prefetch)
# what must show in a KLTTrackFeatures trace at least once: the stage's entry point behind BOTH trackers of a call that repeated its chain
STAGE_ENTRY = {"quality": "klt_track_quality_async", "model": "klt_motion_check_async", "epipolar": "klt_epipolar_check_async",
               "homography": "klt_homography_check_async", "crowd": "klt_crowd_check_async"}


def _norm(a, where=None):
    """one argument as something JSON keeps and that is the same run after run"""
    from pyfeaturetrack_amd.backend import ConsensusCheck
    if isinstance(a, ConsensusCheck):
        return "check:" + a.name
    if isinstance(a, np.ndarray):
        if a.dtype.names is not None:                       # a record array is a download's target: nothing in it yet
            return "array%s rec%d" % (list(a.shape), a.dtype.itemsize)
        return "array%s %s %s" % (list(a.shape), a.dtype.str, a.reshape(-1)[:1].tobytes().hex())
    if isinstance(a, np.dtype) or (isinstance(a, type) and issubclass(a, np.generic)):
        return "dtype:" + np.dtype(a).str
    if isinstance(a, C.Structure):
        return "%s:%s" % (type(a).__name__, bytes(a).hex())
    if isinstance(a, C.Array):
        vals = list(a)
        if vals and isinstance(vals[0], float):
            return "f64[%d]:%s" % (len(vals), hashlib.sha256(bytes(a)).hexdigest()[:12])
        return "%s%s" % (type(a)._type_.__name__, vals)
    if type(a).__name__ == "CArgObject":                     # C.byref(...)
        return _norm(a._obj, where) if isinstance(a._obj, C.Structure) else "out:" + type(a._obj).__name__
    if isinstance(a, C.c_void_p):
        return _norm(a.value, where)
    if isinstance(a, (bool, np.bool_)):
        return bool(a)
    if isinstance(a, (int, np.integer)):
        a = int(a)
        if where is not None and a >= 1 << 32:
            return where(a)
        return a
    if isinstance(a, float):
        return repr(a)
    if a is None or isinstance(a, str):
        return a
    if isinstance(a, (tuple, list)):
        return [_norm(v, where) for v in a]
    return "<%s>" % type(a).__name__


def _entry(name, args, kwargs, where=None):
    parts = [repr(_norm(a, where)) for a in args] + ["%s=%r" % (k, _norm(v, where)) for k, v in sorted(kwargs.items())]
    return "%s(%s)" % (name, ", ".join(parts))


def _tc(stage, **more):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    tc = KLT_TrackingContext()
    for k, v in dict(dict(STAGE_OPTIONS)[stage], **more).items():
        setattr(tc, k, v)
    return tc


def _table_digest(ft):
    """the tables of the result: which are there, of which type and shape, and which of their bytes the call itself zeroed"""
    out = []
    for name in ("quality", "crowd", "models", "epipolar", "homography"):
        t = getattr(ft, name)
        out.append("%s=%s" % (name, None if t is None else "%s%s %s" % (t.dtype.itemsize, list(t.shape), hashlib.sha256(t.tobytes()).hexdigest()[:12])))
    return "result(%d, %d, aux=%s; %s)" % (ft.nFrames, ft.nFeatures, bool((ft.rec["aux"] == 0).all()), "; ".join(out))


# ------------------------------------------------------------------------------------------- KLTTrackSequence on a recording context
class SequenceRecorder:
    """stands in for backend.Context: every method call is logged; the few that have to answer do"""

    def __init__(self):
        self.lock = threading.RLock()
        self.log = []
        self._looks = 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kwargs):
            self.log.append(_entry(name, args, kwargs))
            answer = getattr(type(self), "_answer_" + name, None)
            return None if answer is None else answer(self, *args, **kwargs)
        return call

    def _answer_take_slots(self, n=3):
        return 0

    def _answer_take_affine_state(self):
        return 0

    def _answer_staging(self, shape, count=2, dtype=np.uint8):
        return [np.empty(shape, dtype) for _ in range(count)]

    def _answer_select_finish(self):
        self._looks += 1
        return self._looks % 3 == 0                         # now and then the list was rewritten: the tracker is enqueued again

    def _answer_featbuf_download_into(self, fb, out):
        out.view(np.uint8)[...] = 1                        # (what the call zeroes afterwards shows in the result's digest)

    def _answer_slot_generation(self, slot):
        return 1


def sequence_cases():
    for (stage, _), nframes, arrangement in itertools.product(STAGE_OPTIONS, FRAME_COUNTS, ARRANGEMENTS):
        yield stage, 10, nframes, arrangement
    for nframes, arrangement in itertools.product(FRAME_COUNTS, ARRANGEMENTS):
        yield "all", 0, nframes, arrangement


def sequence_case_name(stage, nfeatures, nframes, arrangement):
    return "%s/n%d/f%d/%s" % (stage, nfeatures, nframes, "".join("FT"[bool(a)] for a in arrangement))


def sequence_trace(stage, nfeatures, nframes, arrangement):
    from pyfeaturetrack_amd import trackSequence as ts
    tc = _tc(stage, sequentialMode=True)
    ctx = SequenceRecorder()
    tc.__dict__["_klt_ctx"] = ctx
    frames = [np.full((H, W), k, np.uint8) for k in range(nframes)]
    ft = ts._track_sequence_locked(ctx, tc, iter(frames), nfeatures, *arrangement)
    return ctx.log + [_table_digest(ft)]


# ------------------------------------------------------------------------------------------- KLTTrackFeatures over a recording library
_FINALIZER_CALLS = ("klt_slot_free", "klt_affine_free", "klt_destroy")          # made when the collector pleases: not part of a trace


class FakeLibrary:
    """stands in for libkltgpu behind a real Context: every klt_* call is logged and answers 0; pinned memory is zeroed host memory,
    downloads bring zeros, and the state of a slot follows the uploads, builds and swaps seen"""

    def __init__(self):
        self.log = []
        self.blocks = []                                    # [(address, size, ctypes buffer)] of klt_host_alloc, in order
        self.state, self.generation, self._builds = {}, {}, 0

    def where(self, address):
        for i, (base, size, _) in enumerate(self.blocks):
            if base <= address < base + size:
                return "host%d+%d" % (i, address - base)
        return "ptr"

    def __getattr__(self, name):
        if not name.startswith("klt_"):
            raise AttributeError(name)

        def call(handle, *args):
            if name not in _FINALIZER_CALLS:
                self.log.append(_entry(name, args, {}, self.where))
            do = getattr(type(self), "_do_" + name, None)
            return 0 if do is None else do(self, *args)
        return call

    def _do_klt_host_alloc(self, nbytes, out):
        buf = (C.c_uint8 * max(1, nbytes))()
        self.blocks.append((C.addressof(buf), nbytes, buf))
        out._obj.value = C.addressof(buf)
        return 0

    def _do_klt_host_free(self, p):
        return 0                                            # (the block keeps its name: the addresses of a trace never clash)

    def _uploaded(self, slot, *rest):
        self.state[slot] = 1
        self.generation[slot] = 0
        return 0
    _do_klt_upload_u8 = _do_klt_upload_f32 = _do_klt_upload_u8_async = _do_klt_upload_f32_async = _uploaded

    def _built(self, slot):
        self._builds += 1
        self.state[slot] = self.state.get(slot, 0) | 2
        self.generation[slot] = self._builds
        return 0
    _do_klt_build_pyramids = _do_klt_build_pyramids_async = _built

    def _do_klt_build_pyramids_batch_async(self, slots, n):
        for s in list(slots)[:n]:
            self._built(s)
        return 0

    def _do_klt_swap_slots(self, a, b):
        for table in (self.state, self.generation):
            table[a], table[b] = table.get(b, 0), table.get(a, 0)
        return 0

    def _do_klt_slot_state(self, slot):
        return self.state.get(slot, 0)

    def _do_klt_slot_generation(self, slot, out):
        out._obj.value = self.generation.get(slot, 0)
        return 0

    def _do_klt_featbuf_download(self, fb, dst, n):
        C.memset(dst, 0, 16 * n)
        return 0

    def _do_klt_affine_download(self, state, dst, n):
        C.memset(dst, 0, 32 * n)
        return 0


def fake_context():
    import collections
    from pyfeaturetrack_amd.backend import Context
    ctx = Context.__new__(Context)
    ctx._lib, ctx._h, ctx.device = FakeLibrary(), C.c_void_p(1), 0
    ctx._params_key, ctx._consensus_keys = None, {}
    ctx.lock, ctx._deferred = threading.RLock(), collections.deque()
    return ctx


FEATURES_STAGES = tuple(s for s, _ in STAGE_OPTIONS) + ("gain_bias",)


def features_cases():
    return itertools.product(FEATURES_STAGES, (True, False), (False, True), (False, True), (True, False))


def features_case_name(stage, sequential, guess, age, map_records):
    return "%s/%s/%s/%s/%s" % (stage, "sequential" if sequential else "pingpong", "guess" if guess else "-", "age" if age else "-",
                               "mapped" if map_records else "copied")


def features_trace(stage, sequential, guess, age, map_records, keep=None):
    """the library calls of three KLTTrackFeatures calls in a row -- ["call k", entries ...] per call, an exception as its text -- the third
    on a frame that the slot seems to hold (same object, same lattice) and does not: the chain behind the tracker runs twice there"""
    from pyfeaturetrack_amd import backend, trackFeatures
    from pyfeaturetrack_amd.klt import new_feature_list
    n = 12
    if stage == "gain_bias":
        tc = _tc("none", lightingCompensation="gain_bias", sequentialMode=sequential)
    else:
        tc = _tc(stage, sequentialMode=sequential)
    ctx = fake_context()
    tc.__dict__["_klt_ctx"] = ctx
    fl = new_feature_list(n, fill=True)
    for i, f in enumerate(fl):
        f.x, f.y, f.val = 8.0 + 4 * i, 10.0 + 2 * i, 0
    rng = np.random.default_rng(7)
    a, b, c = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3))
    pairs = ((a, b), (b, c), (c, b)) if sequential else ((a, b), (b, a), (a, b))
    was_verbose, was_mapped = trackFeatures.KLT_verbose, backend.MAP_RECORDS
    trackFeatures.KLT_verbose, backend.MAP_RECORDS = 0, map_records
    out = []
    try:
        for k, (img1, img2) in enumerate(pairs):
            if k == 2:
                b[5, 7] ^= 1                                # off the 1024-pixel lattice (every second column of a frame this small)
            kw = {}
            if guess:
                kw["guess"] = np.array([[f.x + 0.5, f.y - 0.25] for f in fl], np.float32)
            if age:
                kw["age"] = np.arange(n, dtype=np.int32)
            out.append("call %d" % k)
            try:
                trackFeatures.KLTTrackFeatures(tc, img1, img2, fl, **kw)
            except Exception as e:                          # noqa: BLE001 -- a combination the API refuses is part of the record
                out.append("%s: %s" % (type(e).__name__, e))
            out.extend(ctx._lib.log)
            del ctx._lib.log[:]
            out.append("left(%s)" % ", ".join("%s=%s" % (name, _left(getattr(tc, name, "unset")))
                                              for name in ("quality_last", "crowding_last", "model_last", "epipolar_last", "homography_last")))
    finally:
        trackFeatures.KLT_verbose, backend.MAP_RECORDS = was_verbose, was_mapped
    if keep is not None:
        keep.append((tc, ctx, fl))                          # (until the caller has its trace: their finalizers call into the library)
    return out


def _left(value):
    if isinstance(value, np.ndarray) or isinstance(value, np.void):
        return "%s%s %s" % (value.dtype.itemsize, list(value.shape), hashlib.sha256(value.tobytes()).hexdigest()[:12])
    if isinstance(value, dict):
        return sorted(value)
    return value


def repeats_chain(trace, entry):
    """True when one call of the trace shows a tracker entry point twice, each time followed by `entry` before the next tracker"""
    calls, cur = [], None
    for e in trace:
        if e.startswith("call "):
            cur = []
            calls.append(cur)
        elif cur is not None:
            cur.append(e.split("(")[0])
    for names in calls:
        trackers = [i for i, nm in enumerate(names) if nm.startswith("klt_track") and nm.endswith("_async") and "quality" not in nm]
        if len(trackers) == 2 and all(entry in names[i + 1:(trackers + [len(names)])[j + 1]] for j, i in enumerate(trackers)):
            return True
    return False


# ------------------------------------------------------------------------------------------- the file
def encode(traces):
    """{case: [entries]} -> (strings, {case: [indices] or {"entries": n, "sha256": ...}})"""
    strings, index, out = [], {}, {}
    for name, trace in traces.items():
        if isinstance(trace, dict):
            out[name] = trace
            continue
        ids = []
        for e in trace:
            if e not in index:
                index[e] = len(strings)
                strings.append(e)
            ids.append(index[e])
        out[name] = ids
    return strings, out


def digest(trace):
    return {"entries": len(trace), "sha256": hashlib.sha256("\n".join(trace).encode()).hexdigest()}


def record_all():
    """every case of both kinds, as the golden file keeps it"""
    seq = {}
    for case in sequence_cases():
        t = sequence_trace(*case)
        seq[sequence_case_name(*case)] = t if case[2] <= FULL_TRACE_UP_TO else digest(t)
    keep, feat = [], {}
    for case in features_cases():
        feat[features_case_name(*case)] = features_trace(*case, keep=keep)
    return seq, feat
