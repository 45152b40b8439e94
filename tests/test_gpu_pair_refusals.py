"""What every entry point that takes a frame pair and / or feature buffers ANSWERS to a bad call: the return code and the whole message,
compared with tests/golden/pair_refusals.json -- which fault is reported when a call has two, what n == 0 does on a buffer without memory,
and how many allocation sites a synchronous call has.  The file was recorded on the GPU from the library of commit 27eeaaf (the parent
of the change that gave the launches' host path one copy of each buffer check) by this module's recording mode,

    python tests/test_gpu_pair_refusals.py --record tests/golden/pair_refusals.json

and is not regenerated: the expected values never come from the tree under test.  Every case is answered on the host -- a refusal, or a
no-op that returns KLT_OK (the launchers return before launching when n == 0); none reaches a kernel.  After every case, behind a sync:
code and message equal the recording, the bytes of every feature buffer (and of the host arrays of the synchronous calls) are unchanged,
and the buffers that did not exist still do not (a refused call allocates nothing).  At the end the good calls of the start give the same
bytes again.

The synchronous entry points are called through the ctypes handle: the Context methods copy their arrays, which would hide a refused
call that wrote to its `inout`; so are the calls a method cannot express (n = -1 with an array, a null column)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FILE = os.path.join(HERE, "golden", "pair_refusals.json")
OPT_FAIL_ALLOC_AFTER = 19
N = 16
WIDTH, HEIGHT = 64, 48
# slots: a built pair, a built frame of another size, a frame without pyramids, an index never filled
S0, S1, S_TALL, S_RAW, S_NONE = 0, 1, 2, 3, 7
# feature buffers of two pairs ...
IN, OUT, BACK, GUESS, Q, M = 10, 11, 12, 13, 14, 15
IN2, OUT2, BACK2, GUESS2, Q2, M2 = 20, 21, 22, 23, 24, 25
PREV = 40                                                        # (the highest index in use)
# ... views of their lists, a buffer one record short, an index below PREV that never got memory, two indices never made
V_IN, V_OUT, SHORT, HOLE, V_BACK, V_OUT2, V_IN2, V_Q2 = 31, 32, 33, 34, 35, 36, 37, 38
NEVER, NEVER2 = 50, 51
OWNED = {IN: N, OUT: N, BACK: N, GUESS: N, Q: N, M: N, IN2: N, OUT2: N, BACK2: N, GUESS2: N, Q2: N, M2: N, PREV: N, SHORT: N - 1}
ABSENT = (HOLE, NEVER, NEVER2)
STATE, NO_STATE = 0, 5                                           # affine states: allocated for N features, never allocated

_ERR = re.compile(r"libkltgpu error (-?\d+): (.*)\Z", re.S)


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def feature_lists():
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    rng = np.random.RandomState(7)
    lists = []
    for _ in range(2):
        fl = np.zeros(N, FEAT_DTYPE)
        fl["x"] = (14 + 36 * rng.rand(N)).astype(np.float32)
        fl["y"] = (14 + 20 * rng.rand(N)).astype(np.float32)
        fl["val"] = 1
        lists.append(fl)
    return lists


def shifted(fl, dx, dy):
    out = fl.copy()
    out["x"] += np.float32(dx)
    out["y"] += np.float32(dy)
    return out


def load_frames(ctx):
    from helpers import make_tc
    from pyfeaturetrack_amd import synth
    ctx.configure(make_tc(levels=2, ss=2, window=7))
    ctx.set_light_params(mode=0)
    ctx.set_fb_params(max_error=1.0)
    f0, f1 = synth.synth_pair(WIDTH, HEIGHT, seed=3)
    tall, _ = synth.synth_pair(HEIGHT, WIDTH, seed=3)
    for slot, frame, built in ((S0, f0, True), (S1, f1, True), (S_TALL, tall, True), (S_RAW, f0, False)):
        ctx.upload(slot, frame)
        if built:
            ctx.build_pyramids(slot)


def affine_params(mode):
    from pyfeaturetrack_amd._abi import KltAffineParams
    return KltAffineParams(mode, 15, 15, 10, 10.0, 0.02, 1.5)       # (the tracking context's defaults: configure() sets the same window)


def build_world(ctx):
    load_frames(ctx)
    ctx.set_model_params(mode=1, ncols=WIDTH, nrows=HEIGHT)
    fl, fl2 = feature_lists()
    ctx.featbuf_upload(IN, fl)
    ctx.featbuf_upload(IN2, fl2)
    ctx.featbuf_upload(GUESS, shifted(fl, 1.0, -0.5))
    ctx.featbuf_upload(GUESS2, shifted(fl2, 1.0, -0.5))
    ctx.featbuf_upload(PREV, shifted(fl, -1.0, 0.5))
    for fb in (OUT, BACK, Q, M, OUT2, BACK2, Q2, M2):
        ctx.featbuf_alloc(fb, N)
    ctx.featbuf_alloc(SHORT, N - 1)
    for view, parent in ((V_IN, IN), (V_OUT, OUT), (V_BACK, BACK), (V_OUT2, OUT2), (V_IN2, IN2), (V_Q2, Q2)):
        ctx.featbuf_view(view, parent, 0, N)
    ctx.set_affine_params(affine_params(1))
    ctx.affine_alloc(STATE, N)
    ctx.set_affine_params(affine_params(-1))
    ctx.sync()
    return fl, fl2


def snapshot(ctx):
    ctx.sync()
    return {fb: ctx.featbuf_download(fb, cap).tobytes() for fb, cap in OWNED.items()}


def good_calls(ctx):
    """one call each of track, fb, guess, quality (single and a batch of 2) and model (single and a batch of 2): behind each, the bytes of
    the buffers it writes"""
    shots = []
    for call, written in ((lambda: ctx.track_async(S0, S1, IN2, OUT2, N), (OUT2,)),
                          (lambda: ctx.track_async(S0, S1, IN, OUT, N), (OUT,)),
                          (lambda: ctx.track_fb_async(S0, S1, IN, OUT, N, BACK), (OUT, BACK)),
                          (lambda: ctx.track_guess_async(S0, S1, IN, GUESS, OUT, N), (OUT,)),
                          (lambda: ctx.track_quality_async(S0, S1, IN, OUT, Q, N), (Q,)),
                          (lambda: ctx.track_quality_batch_async([(S0, S1, IN, OUT, Q), (S0, S1, IN2, OUT2, Q2)], N), (Q, Q2)),
                          (lambda: ctx.motion_check_async(IN, OUT, M, N), (OUT, M)),
                          (lambda: ctx.motion_check_batch_async([(IN, OUT, M), (IN2, OUT2, M2)], N), (OUT, OUT2, M, M2))):
        call()
        shot = snapshot(ctx)
        shots.append({fb: shot[fb] for fb in written})
    return shots


def make_cases(ctx, host):
    """[(name, thunk)]: a thunk makes one call and returns None (a Context method that came back: KLT_OK) or (code, message) of a call
    through the ctypes handle; a refused Context method raises"""
    from pyfeaturetrack_amd._abi import KltMotionModel
    lib, h = ctx._lib, ctx._h
    cases = []

    def add(name, fn):
        cases.append((name, fn))

    def raw(name, *args):
        def run():
            rc = getattr(lib, name)(h, *args)
            return rc, ((lib.klt_last_error(h) or b"").decode() if rc < 0 else "")
        return run

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def during(enter, leave, fn):
        def run():
            enter()
            try:
                return fn()
            finally:
                leave()
        return run

    def lit(fn):                                                 # lighting mode 1 for the length of the call
        return during(lambda: ctx.set_light_params(mode=1), lambda: ctx.set_light_params(mode=0), fn)

    def model_off(fn):
        return during(lambda: ctx.set_model_params(mode=0, ncols=WIDTH, nrows=HEIGHT),
                      lambda: ctx.set_model_params(mode=1, ncols=WIDTH, nrows=HEIGHT), fn)

    def affine_on(fn):
        return during(lambda: ctx.set_affine_params(affine_params(1)), lambda: ctx.set_affine_params(affine_params(-1)), fn)

    def slot_faults(p, f):
        add(p + ".slot_never_filled", f(S0, S_NONE))
        add(p + ".slot_without_pyramids", f(S0, S_RAW))
        add(p + ".pair_of_two_sizes", f(S0, S_TALL))

    LISTS = ((-1, "-1"), (65536, "65536"), (HOLE, "without_memory"), (NEVER, "never_made"), (SHORT, "short"))
    RANGE = ((-1, "-1"), (65536, "65536"))

    def T(*a): return lambda: ctx.track_async(*a)                              # slot1, slot2, in, out, n
    def TF(*a): return lambda: ctx.track_fb_async(*a)                          # slot1, slot2, in, out, n, back
    def TG(*a): return lambda: ctx.track_guess_async(*a)                       # slot1, slot2, in, guess, out, n
    def TFG(*a): return lambda: ctx.track_fb_guess_async(*a)                   # slot1, slot2, in, guess, out, n, back
    def PCV(*a): return lambda: ctx.predict_cv_async(*a)                       # prev, cur, guess, n
    def TB(pairs, n): return lambda: ctx.track_batch_async(pairs, n)           # [(slot1, slot2, in, out)]
    def TFB(pairs, n): return lambda: ctx.track_fb_batch_async(pairs, n)       # [(slot1, slot2, in, out[, back])]
    def TGB(pairs, n): return lambda: ctx.track_guess_batch_async(pairs, n)    # [(slot1, slot2, in, guess, out)]
    def QA(*a): return lambda: ctx.track_quality_async(*a)                     # slot1, slot2, in, out, q, n
    def QB(pairs, n): return lambda: ctx.track_quality_batch_async(pairs, n)   # [(slot1, slot2, in, out, q)]
    def MA(*a): return lambda: ctx.motion_check_async(*a)                      # in, out, model, n
    def MB(pairs, n): return lambda: ctx.motion_check_batch_async(pairs, n)    # [(in, out, model)]
    def TA(*a): return lambda: ctx.track_affine_async(*a)                      # slot1, slot2, in, out, n, state

    # ---------------------------------------------------------------- klt_track_async
    p = "track_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), T(S0, S1, bad, OUT, N))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), T(S0, S1, IN, bad, N))
    slot_faults(p, lambda a, b: T(a, b, IN, OUT, N))
    add(p + ".n_-1", T(S0, S1, IN, OUT, -1))
    add(p + ".two.out_65536+slot_without_pyramids", T(S0, S_RAW, IN, 65536, N))
    add(p + ".two.in_short+pair_of_two_sizes", T(S0, S_TALL, SHORT, OUT, N))
    add(p + ".n0.in_without_memory", T(S0, S1, HOLE, OUT, 0))
    add(p + ".n0.in_never_made", T(S0, S1, NEVER, OUT, 0))

    # ---------------------------------------------------------------- klt_track_fb_async
    p = "track_fb_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TF(S0, S1, bad, OUT, N, BACK))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TF(S0, S1, IN, bad, N, BACK))
    add(p + ".back_-2", TF(S0, S1, IN, OUT, N, -2))
    add(p + ".back_65536", TF(S0, S1, IN, OUT, N, 65536))
    add(p + ".in_is_out", TF(S0, S1, IN, IN, N, BACK))
    add(p + ".back_is_in", TF(S0, S1, IN, OUT, N, IN))
    add(p + ".back_is_out", TF(S0, S1, IN, OUT, N, OUT))
    slot_faults(p, lambda a, b: TF(a, b, IN, OUT, N, BACK))
    add(p + ".n_-1", TF(S0, S1, IN, OUT, -1, BACK))
    add(p + ".lighting", lit(TF(S0, S1, IN, OUT, N, BACK)))
    add(p + ".two.back_is_out+slot_without_pyramids", TF(S0, S_RAW, IN, OUT, N, OUT))
    add(p + ".two.lighting+n_-1", lit(TF(S0, S1, IN, OUT, -1, BACK)))
    add(p + ".n0.in_without_memory", TF(S0, S1, HOLE, OUT, 0, BACK))

    # ---------------------------------------------------------------- klt_track_guess_async
    p = "track_guess_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TG(S0, S1, bad, GUESS, OUT, N))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TG(S0, S1, IN, GUESS, bad, N))
        add("%s.guess_%s" % (p, tag), TG(S0, S1, IN, bad, OUT, N))
    add(p + ".guess_is_out", TG(S0, S1, IN, OUT, OUT, N))
    add(p + ".guess_views_out", TG(S0, S1, IN, V_OUT, OUT, N))
    for bad, tag in LISTS[2:]:
        add("%s.guess_%s" % (p, tag), TG(S0, S1, IN, bad, OUT, N))
    slot_faults(p, lambda a, b: TG(a, b, IN, GUESS, OUT, N))
    add(p + ".n_-1", TG(S0, S1, IN, GUESS, OUT, -1))
    add(p + ".lighting", lit(TG(S0, S1, IN, GUESS, OUT, N)))
    add(p + ".two.guess_is_out+slot_without_pyramids", TG(S0, S_RAW, IN, OUT, OUT, N))
    add(p + ".two.guess_short+slot_without_pyramids", TG(S0, S_RAW, IN, SHORT, OUT, N))
    add(p + ".n0.in_without_memory", TG(S0, S1, HOLE, GUESS, OUT, 0))
    add(p + ".n0.guess_without_memory", TG(S0, S1, IN, HOLE, OUT, 0))

    # ---------------------------------------------------------------- klt_track_fb_guess_async
    p = "track_fb_guess_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TFG(S0, S1, bad, GUESS, OUT, N, BACK))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TFG(S0, S1, IN, GUESS, bad, N, BACK))
        add("%s.guess_%s" % (p, tag), TFG(S0, S1, IN, bad, OUT, N, BACK))
    add(p + ".back_-2", TFG(S0, S1, IN, GUESS, OUT, N, -2))
    add(p + ".back_65536", TFG(S0, S1, IN, GUESS, OUT, N, 65536))
    add(p + ".in_is_out", TFG(S0, S1, IN, GUESS, IN, N, BACK))
    add(p + ".guess_is_out", TFG(S0, S1, IN, OUT, OUT, N, BACK))
    add(p + ".guess_is_back", TFG(S0, S1, IN, BACK, OUT, N, BACK))
    add(p + ".guess_views_out", TFG(S0, S1, IN, V_OUT, OUT, N, BACK))
    add(p + ".guess_views_back", TFG(S0, S1, IN, V_BACK, OUT, N, BACK))
    for bad, tag in LISTS[2:]:
        add("%s.guess_%s" % (p, tag), TFG(S0, S1, IN, bad, OUT, N, BACK))
    slot_faults(p, lambda a, b: TFG(a, b, IN, GUESS, OUT, N, BACK))
    add(p + ".n_-1", TFG(S0, S1, IN, GUESS, OUT, -1, BACK))
    add(p + ".lighting", lit(TFG(S0, S1, IN, GUESS, OUT, N, BACK)))
    add(p + ".two.guess_is_back+slot_without_pyramids", TFG(S0, S_RAW, IN, BACK, OUT, N, BACK))
    add(p + ".two.lighting+guess_-1", lit(TFG(S0, S1, IN, -1, OUT, N, BACK)))
    add(p + ".n0.in_without_memory", TFG(S0, S1, HOLE, GUESS, OUT, 0, BACK))

    # ---------------------------------------------------------------- klt_predict_cv_async
    p = "predict_cv_async"
    for bad, tag in LISTS:
        add("%s.prev_%s" % (p, tag), PCV(bad, IN, GUESS, N))
        add("%s.cur_%s" % (p, tag), PCV(PREV, bad, GUESS, N))
    for bad, tag in RANGE:
        add("%s.guess_%s" % (p, tag), PCV(PREV, IN, bad, N))
    add(p + ".guess_is_prev", PCV(PREV, IN, PREV, N))
    add(p + ".guess_is_cur", PCV(PREV, IN, IN, N))
    add(p + ".guess_views_cur", PCV(PREV, IN, V_IN, N))
    add(p + ".n_-1", PCV(PREV, IN, GUESS, -1))
    add(p + ".two.guess_is_cur+prev_without_memory", PCV(HOLE, IN, IN, N))
    add(p + ".two.guess_65536+prev_short", PCV(SHORT, IN, 65536, N))
    add(p + ".n0.prev_without_memory", PCV(HOLE, IN, GUESS, 0))
    add(p + ".n0.cur_without_memory", PCV(PREV, HOLE, GUESS, 0))

    # ---------------------------------------------------------------- klt_track_batch_async
    p = "track_batch_async"
    A, B = (S0, S1, IN, OUT), (S0, S1, IN2, OUT2)
    add(p + ".empty_batch", TB([], N))
    add(p + ".n_-1", TB([A, B], -1))
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TB([A, (S0, S1, bad, OUT2)], N))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TB([A, (S0, S1, IN2, bad)], N))
    slot_faults(p, lambda a, b: TB([A, (a, b, IN2, OUT2)], N))
    add(p + ".pairs_of_two_frame_sizes", TB([A, (S_TALL, S_TALL, IN2, OUT2)], N))
    add(p + ".two.out_65536+slot_without_pyramids", TB([(S0, S_RAW, IN, OUT), (S0, S1, IN2, 65536)], N))
    add(p + ".two.in_short+pair_of_two_sizes", TB([(S0, S1, SHORT, OUT), (S0, S_TALL, IN2, OUT2)], N))
    add(p + ".n0.in_without_memory", TB([A, (S0, S1, HOLE, OUT2)], 0))
    add(p + ".n0.in_never_made", TB([A, (S0, S1, NEVER, OUT2)], 0))

    # ---------------------------------------------------------------- klt_track_fb_batch_async
    p = "track_fb_batch_async"
    A, B = (S0, S1, IN, OUT, BACK), (S0, S1, IN2, OUT2, BACK2)
    add(p + ".empty_batch", TFB([], N))
    add(p + ".n_-1", TFB([A, B], -1))
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TFB([A, (S0, S1, bad, OUT2, BACK2)], N))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TFB([A, (S0, S1, IN2, bad, BACK2)], N))
    add(p + ".back_-2", TFB([A, (S0, S1, IN2, OUT2, -2)], N))
    add(p + ".back_65536", TFB([A, (S0, S1, IN2, OUT2, 65536)], N))
    add(p + ".in_is_out", TFB([A, (S0, S1, IN2, IN2, BACK2)], N))
    add(p + ".back_is_in", TFB([A, (S0, S1, IN2, OUT2, IN2)], N))
    add(p + ".back_is_out", TFB([A, (S0, S1, IN2, OUT2, OUT2)], N))
    slot_faults(p, lambda a, b: TFB([A, (a, b, IN2, OUT2, BACK2)], N))
    add(p + ".pairs_of_two_frame_sizes", TFB([A, (S_TALL, S_TALL, IN2, OUT2, BACK2)], N))
    add(p + ".lighting", lit(TFB([A, B], N)))
    add(p + ".two.back_is_out+slot_without_pyramids", TFB([(S0, S_RAW, IN, OUT, BACK), (S0, S1, IN2, OUT2, OUT2)], N))
    add(p + ".two.lighting+empty_batch", lit(TFB([], N)))
    add(p + ".n0.in_without_memory", TFB([A, (S0, S1, HOLE, OUT2, BACK2)], 0))

    # ---------------------------------------------------------------- klt_track_guess_batch_async
    p = "track_guess_batch_async"
    A, B = (S0, S1, IN, GUESS, OUT), (S0, S1, IN2, GUESS2, OUT2)
    add(p + ".empty_batch", TGB([], N))
    add(p + ".n_-1", TGB([A, B], -1))
    add(p + ".null_guess_column", raw("klt_track_guess_batch_async", ints(S0, S0), ints(S1, S1), ints(IN, IN2), None, ints(OUT, OUT2), 2, N))
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), TGB([A, (S0, S1, bad, GUESS2, OUT2)], N))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), TGB([A, (S0, S1, IN2, GUESS2, bad)], N))
    add(p + ".guess_-2", TGB([A, (S0, S1, IN2, -2, OUT2)], N))
    add(p + ".guess_65536", TGB([A, (S0, S1, IN2, 65536, OUT2)], N))
    add(p + ".guess_is_own_out", TGB([A, (S0, S1, IN2, OUT2, OUT2)], N))
    add(p + ".guess_is_other_pairs_out", TGB([(S0, S1, IN, OUT2, OUT), B], N))
    add(p + ".guess_views_own_out", TGB([(S0, S1, IN, V_OUT, OUT), B], N))
    add(p + ".guess_views_other_pairs_out", TGB([(S0, S1, IN, V_OUT2, OUT), B], N))
    for bad, tag in LISTS[2:]:
        add("%s.guess_%s" % (p, tag), TGB([A, (S0, S1, IN2, bad, OUT2)], N))
    slot_faults(p, lambda a, b: TGB([A, (a, b, IN2, GUESS2, OUT2)], N))
    add(p + ".pairs_of_two_frame_sizes", TGB([A, (S_TALL, S_TALL, IN2, GUESS2, OUT2)], N))
    add(p + ".lighting", lit(TGB([A, B], N)))
    add(p + ".two.guess_is_other_pairs_out+slot_without_pyramids", TGB([(S0, S_RAW, IN, OUT2, OUT), B], N))
    add(p + ".two.guess_short+in_short", TGB([A, (S0, S1, SHORT, SHORT, OUT2)], N))
    add(p + ".n0.in_without_memory", TGB([A, (S0, S1, HOLE, GUESS2, OUT2)], 0))
    add(p + ".n0.guess_without_memory", TGB([A, (S0, S1, IN2, HOLE, OUT2)], 0))

    # ---------------------------------------------------------------- klt_track_quality_async
    p = "track_quality_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), QA(S0, S1, bad, OUT, Q, N))
        add("%s.out_%s" % (p, tag), QA(S0, S1, IN, bad, Q, N))
    for bad, tag in RANGE:
        add("%s.q_%s" % (p, tag), QA(S0, S1, IN, OUT, bad, N))
    add(p + ".q_is_in", QA(S0, S1, IN, OUT, IN, N))
    add(p + ".q_is_out", QA(S0, S1, IN, OUT, OUT, N))
    add(p + ".q_views_in", QA(S0, S1, IN, OUT, V_IN, N))
    add(p + ".q_views_out", QA(S0, S1, IN, OUT, V_OUT, N))
    slot_faults(p, lambda a, b: QA(a, b, IN, OUT, Q, N))
    add(p + ".n_-1", QA(S0, S1, IN, OUT, Q, -1))
    add(p + ".in_short.q_never_made", QA(S0, S1, SHORT, OUT, NEVER, N))
    add(p + ".two.q_is_in+slot_without_pyramids", QA(S0, S_RAW, IN, OUT, IN, N))
    add(p + ".two.q_views_in+slot_without_pyramids", QA(S0, S_RAW, IN, OUT, V_IN, N))
    add(p + ".two.q_views_out+in_short", QA(S0, S1, SHORT, OUT, V_OUT, N))
    add(p + ".n0.in_without_memory.q_never_made", QA(S0, S1, HOLE, OUT, NEVER, 0))

    # ---------------------------------------------------------------- klt_track_quality_batch_async
    p = "track_quality_batch_async"
    A, B = (S0, S1, IN, OUT, Q), (S0, S1, IN2, OUT2, Q2)
    add(p + ".empty_batch", QB([], N))
    add(p + ".n_-1", QB([A, B], -1))
    add(p + ".null_q_column", raw("klt_track_quality_batch_async", ints(S0, S0), ints(S1, S1), ints(IN, IN2), ints(OUT, OUT2), None, 2, N))
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), QB([A, (S0, S1, bad, OUT2, Q2)], N))
        add("%s.out_%s" % (p, tag), QB([A, (S0, S1, IN2, bad, Q2)], N))
    for bad, tag in RANGE:
        add("%s.q_%s" % (p, tag), QB([A, (S0, S1, IN2, OUT2, bad)], N))
    add(p + ".q_is_own_in", QB([A, (S0, S1, IN2, OUT2, IN2)], N))
    add(p + ".q_is_own_out", QB([A, (S0, S1, IN2, OUT2, OUT2)], N))
    add(p + ".q_is_other_pairs_in", QB([(S0, S1, IN, OUT, IN2), B], N))
    add(p + ".q_is_other_pairs_out", QB([(S0, S1, IN, OUT, OUT2), B], N))
    add(p + ".two_pairs_share_q", QB([A, (S0, S1, IN2, OUT2, Q)], N))
    add(p + ".q_views_own_out", QB([(S0, S1, IN, OUT, V_OUT), B], N))
    add(p + ".q_views_other_pairs_in", QB([(S0, S1, IN, OUT, V_IN2), B], N))
    add(p + ".q_views_other_pairs_q", QB([(S0, S1, IN, OUT, V_Q2), B], N))
    slot_faults(p, lambda a, b: QB([A, (a, b, IN2, OUT2, Q2)], N))
    add(p + ".pairs_of_two_frame_sizes", QB([A, (S_TALL, S_TALL, IN2, OUT2, Q2)], N))
    add(p + ".in_short.q_never_made", QB([(S0, S1, IN, OUT, NEVER), (S0, S1, SHORT, OUT2, NEVER2)], N))
    add(p + ".two.two_pairs_share_q+slot_without_pyramids", QB([(S0, S_RAW, IN, OUT, Q), (S0, S1, IN2, OUT2, Q)], N))
    add(p + ".two.q_views_other_pairs_in+in_short", QB([(S0, S1, IN, OUT, V_IN2), (S0, S1, SHORT, OUT2, Q2)], N))
    add(p + ".n0.in_without_memory", QB([A, (S0, S1, HOLE, OUT2, Q2)], 0))
    add(p + ".n0.q_never_made", QB([(S0, S1, IN, OUT, NEVER), (S0, S1, IN2, OUT2, NEVER2)], 0))

    # ---------------------------------------------------------------- klt_motion_check_async
    p = "motion_check_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), MA(bad, OUT, M, N))
        add("%s.out_%s" % (p, tag), MA(IN, bad, M, N))
    for bad, tag in RANGE:
        add("%s.model_%s" % (p, tag), MA(IN, OUT, bad, N))
    add(p + ".model_is_in", MA(IN, OUT, IN, N))
    add(p + ".model_is_out", MA(IN, OUT, OUT, N))
    add(p + ".in_is_out", MA(IN, IN, M, N))
    add(p + ".model_views_in", MA(IN, OUT, V_IN, N))
    add(p + ".model_views_out", MA(IN, OUT, V_OUT, N))
    add(p + ".out_views_in", MA(IN, V_IN, M, N))
    add(p + ".n_-1", MA(IN, OUT, M, -1))
    add(p + ".switched_off", model_off(MA(IN, OUT, M, N)))
    add(p + ".in_short.model_never_made", MA(SHORT, OUT, NEVER, N))
    add(p + ".two.model_is_in+switched_off", model_off(MA(IN, OUT, IN, N)))
    add(p + ".two.model_views_out+in_short", MA(SHORT, OUT, V_OUT, N))
    add(p + ".n0.in_without_memory.model_never_made", MA(HOLE, OUT, NEVER, 0))
    add(p + ".n0.switched_off", model_off(MA(IN, OUT, M, 0)))

    # ---------------------------------------------------------------- klt_motion_check_batch_async
    p = "motion_check_batch_async"
    A, B = (IN, OUT, M), (IN2, OUT2, M2)
    add(p + ".empty_batch", MB([], N))
    add(p + ".n_-1", MB([A, B], -1))
    add(p + ".null_model_column", raw("klt_motion_check_batch_async", ints(IN, IN2), ints(OUT, OUT2), None, 2, N))
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), MB([A, (bad, OUT2, M2)], N))
        add("%s.out_%s" % (p, tag), MB([A, (IN2, bad, M2)], N))
    for bad, tag in RANGE:
        add("%s.model_%s" % (p, tag), MB([A, (IN2, OUT2, bad)], N))
    add(p + ".model_is_own_in", MB([A, (IN2, OUT2, IN2)], N))
    add(p + ".model_is_other_pairs_in", MB([(IN, OUT, IN2), B], N))
    add(p + ".model_is_other_pairs_out", MB([(IN, OUT, OUT2), B], N))
    add(p + ".two_pairs_share_model", MB([A, (IN2, OUT2, M)], N))
    add(p + ".in_is_out", MB([A, (IN2, IN2, M2)], N))
    add(p + ".out_is_other_pairs_in", MB([(IN, IN2, M), B], N))
    add(p + ".two_pairs_share_out", MB([A, (IN2, OUT, M2)], N))
    add(p + ".model_views_other_pairs_in", MB([(IN, OUT, V_IN2), B], N))
    add(p + ".out_views_other_pairs_in", MB([(IN, V_IN2, M), B], N))
    add(p + ".switched_off", model_off(MB([A, B], N)))
    add(p + ".in_short.model_never_made", MB([(IN, OUT, NEVER), (SHORT, OUT2, NEVER2)], N))
    add(p + ".two.two_pairs_share_model+switched_off", model_off(MB([A, (IN2, OUT2, M)], N)))
    add(p + ".two.model_views_other_pairs_in+in_short", MB([(IN, OUT, V_IN2), (SHORT, OUT2, M2)], N))
    add(p + ".n0.in_without_memory.model_never_made", MB([(IN, OUT, NEVER), (HOLE, OUT2, NEVER2)], 0))
    add(p + ".n0.switched_off", model_off(MB([A, B], 0)))

    # ---------------------------------------------------------------- klt_track_affine_async (the check switched on unless the name says off)
    p = "track_affine_async"
    for bad, tag in LISTS:
        add("%s.in_%s" % (p, tag), affine_on(TA(S0, S1, bad, OUT, N, STATE)))
    for bad, tag in RANGE:
        add("%s.out_%s" % (p, tag), affine_on(TA(S0, S1, IN, bad, N, STATE)))
    add(p + ".in_is_out", affine_on(TA(S0, S1, IN, IN, N, STATE)))
    add(p + ".check_off.in_is_out", TA(S0, S1, IN, IN, N, STATE))
    add(p + ".no_state", affine_on(TA(S0, S1, IN, OUT, N, NO_STATE)))
    add(p + ".state_-1", affine_on(TA(S0, S1, IN, OUT, N, -1)))
    slot_faults(p, lambda a, b: affine_on(TA(a, b, IN, OUT, N, STATE)))
    add(p + ".n_-1", affine_on(TA(S0, S1, IN, OUT, -1, STATE)))
    add(p + ".lighting", lit(affine_on(TA(S0, S1, IN, OUT, N, STATE))))
    add(p + ".two.in_is_out+no_state", affine_on(TA(S0, S1, IN, IN, N, NO_STATE)))
    add(p + ".two.no_state+out_65536", affine_on(TA(S0, S1, IN, 65536, N, NO_STATE)))
    add(p + ".two.lighting+in_is_out", lit(affine_on(TA(S0, S1, IN, IN, N, STATE))))
    add(p + ".n0.in_without_memory", affine_on(TA(S0, S1, HOLE, OUT, 0, STATE)))

    # ---------------------------------------------------------------- the synchronous entry points (last: their staging buffers sit at the
    # top of the index range, so from here on no index lies beyond the context's table of buffers)
    hin, hout, hguess, hback, hq = (host[k].ctypes.data for k in ("in", "out", "guess", "back", "q"))
    model = C.cast(host["model"].ctypes.data, C.POINTER(KltMotionModel))
    count = C.byref(host["count"])

    p = "track"
    slot_faults(p, lambda a, b: raw("klt_track", a, b, hin, N, count))
    add(p + ".n_-1", raw("klt_track", S0, S1, hin, -1, count))
    add(p + ".null_list", raw("klt_track", S0, S1, None, N, count))
    add(p + ".two.n_-1+slot_without_pyramids", raw("klt_track", S0, S_RAW, hin, -1, count))
    add(p + ".n0", raw("klt_track", S0, S1, hin, 0, count))

    p = "track_fb"
    slot_faults(p, lambda a, b: raw("klt_track_fb", a, b, hin, hback, N, count))
    add(p + ".n_-1", raw("klt_track_fb", S0, S1, hin, hback, -1, count))
    add(p + ".null_list", raw("klt_track_fb", S0, S1, None, hback, N, count))
    add(p + ".lighting", lit(raw("klt_track_fb", S0, S1, hin, hback, N, count)))
    add(p + ".two.lighting+n_-1", lit(raw("klt_track_fb", S0, S1, hin, hback, -1, count)))

    p = "track_guess"
    slot_faults(p, lambda a, b: raw("klt_track_guess", a, b, hin, hguess, N, count))
    add(p + ".n_-1", raw("klt_track_guess", S0, S1, hin, hguess, -1, count))
    add(p + ".null_guess", raw("klt_track_guess", S0, S1, hin, None, N, count))
    add(p + ".lighting", lit(raw("klt_track_guess", S0, S1, hin, hguess, N, count)))
    add(p + ".two.null_guess+lighting", lit(raw("klt_track_guess", S0, S1, hin, None, N, count)))

    p = "track_affine"
    slot_faults(p, lambda a, b: affine_on(raw("klt_track_affine", a, b, hin, N, STATE, count)))
    add(p + ".n_-1", affine_on(raw("klt_track_affine", S0, S1, hin, -1, STATE, count)))
    add(p + ".null_list", affine_on(raw("klt_track_affine", S0, S1, None, N, STATE, count)))
    add(p + ".no_state", affine_on(raw("klt_track_affine", S0, S1, hin, N, NO_STATE, count)))
    add(p + ".lighting", lit(affine_on(raw("klt_track_affine", S0, S1, hin, N, STATE, count))))
    add(p + ".two.n_-1+no_state", affine_on(raw("klt_track_affine", S0, S1, hin, -1, NO_STATE, count)))

    p = "track_quality"
    slot_faults(p, lambda a, b: raw("klt_track_quality", a, b, hin, hout, hq, N))
    add(p + ".n_-1", raw("klt_track_quality", S0, S1, hin, hout, hq, -1))
    add(p + ".null_q", raw("klt_track_quality", S0, S1, hin, hout, None, N))
    add(p + ".two.n_-1+slot_without_pyramids", raw("klt_track_quality", S0, S_RAW, hin, hout, hq, -1))
    add(p + ".n0", raw("klt_track_quality", S0, S1, hin, hout, hq, 0))

    p = "motion_check"
    add(p + ".n_-1", raw("klt_motion_check", hin, hout, model, -1, count))
    add(p + ".null_model", raw("klt_motion_check", hin, hout, None, N, count))
    add(p + ".switched_off", model_off(raw("klt_motion_check", hin, hout, model, N, count)))
    add(p + ".two.n_-1+switched_off", model_off(raw("klt_motion_check", hin, hout, model, -1, count)))
    add(p + ".n0", raw("klt_motion_check", hin, hout, model, 0, count))
    add(p + ".n0.switched_off", model_off(raw("klt_motion_check", hin, hout, model, 0, count)))

    names = [name for name, _ in cases]
    assert len(set(names)) == len(names), "case names repeat"
    return cases


def answer(fn):
    from pyfeaturetrack_amd._abi import KltBackendError
    try:
        r = fn()
    except KltBackendError as e:
        m = _ERR.match(str(e))
        return int(m.group(1)), m.group(2)
    return (0, "") if r is None else r


def run_cases(ctx):
    """every case against the world, the invariants asserted behind each: [{"name", "rc", "message"}]"""
    from pyfeaturetrack_amd.backend import MODEL_DTYPE
    fl, _ = build_world(ctx)
    first = good_calls(ctx)
    tracked = np.frombuffer(first[1][OUT], fl.dtype)             # what klt_track_async made of the list
    host = {"in": fl.copy(), "out": tracked.copy(), "guess": shifted(fl, 1.0, -0.5), "back": np.zeros(N, fl.dtype), "q": np.zeros(N, fl.dtype),
            "model": np.zeros(1, MODEL_DTYPE), "count": C.c_int(-7)}
    arrays = ("in", "out", "guess", "back", "q", "model")
    host_before = {k: host[k].tobytes() for k in arrays}
    before = snapshot(ctx)
    answers = []
    for name, fn in make_cases(ctx, host):
        rc, message = answer(fn)
        assert rc <= 0, (name, rc)
        after = snapshot(ctx)
        for fb in OWNED:
            assert after[fb] == before[fb], "%s changed feature buffer %d" % (name, fb)
        for fb in ABSENT:
            assert not ctx.featbuf_devptr(fb), "%s gave feature buffer %d memory" % (name, fb)
        for k in arrays:
            assert host[k].tobytes() == host_before[k], "%s wrote to the caller's `%s`" % (name, k)
        assert host["count"].value == -7 or rc == 0, "%s wrote a count" % name
        host["count"].value = -7
        answers.append({"name": name, "rc": rc, "message": message})
    again = good_calls(ctx)
    for k, (a, b) in enumerate(zip(first, again)):
        assert a == b, "good call %d gives other bytes after the refused calls" % k
    return answers


def allocation_walk(call):
    """how many times in a row a call on a fresh context is refused when its k-th allocation fails, k = 0, 1, ... (the loop of
    test_gpu_guess.py::test_error_paths)"""
    from pyfeaturetrack_amd._abi import KltOutOfMemory
    from pyfeaturetrack_amd.backend import Context
    fresh = Context(0)
    try:
        load_frames(fresh)
        fresh.set_model_params(mode=1, ncols=WIDTH, nrows=HEIGHT)
        refused = 0
        for k in range(16):
            fresh.set_option(OPT_FAIL_ALLOC_AFTER, k)
            try:
                got = call(fresh)
            except KltOutOfMemory:
                refused += 1
                continue
            finally:
                fresh.set_option(OPT_FAIL_ALLOC_AFTER, -1)
            break
        else:
            raise AssertionError("the call never got through")
        return refused, got
    finally:
        fresh.close()


def checked(out, model, n_outliers):
    """what klt_motion_check gave, as one array of bytes"""
    return np.frombuffer(out.tobytes() + model.tobytes(), np.uint8)


def run_walks(ctx):
    load_frames(ctx)
    ctx.set_model_params(mode=1, ncols=WIDTH, nrows=HEIGHT)
    fl, _ = feature_lists()
    guess = shifted(fl, 1.0, -0.5)
    out, _ = ctx.track(S0, S1, fl)
    calls = {"track_guess": lambda c: c.track_guess(S0, S1, fl, guess)[0],
             "track_quality": lambda c: c.track_quality(S0, S1, fl, out),
             "motion_check": lambda c: checked(*c.motion_check(fl, out))}
    counts = {}
    for name, call in calls.items():
        want = call(ctx)
        counts[name], got = allocation_walk(call)
        assert got.tobytes() == want.tobytes(), "%s after %d refused allocations" % (name, counts[name])
    return counts


def test_every_bad_call_answers_as_recorded(ctx, recorded):
    answers = run_cases(ctx)
    want = recorded["cases"]
    assert [a["name"] for a in answers] == [w["name"] for w in want], "the cases are not the recorded ones"
    wrong = ["%s: got (%d, %r), recorded (%d, %r)" % (a["name"], a["rc"], a["message"], w["rc"], w["message"])
             for a, w in zip(answers, want) if (a["rc"], a["message"]) != (w["rc"], w["message"])]
    print("%d cases, %d of them KLT_OK no-ops" % (len(answers), sum(a["rc"] == 0 for a in answers)))
    assert not wrong, "\n".join(wrong)


def test_allocation_walks_as_recorded(ctx, recorded):
    counts = run_walks(ctx)
    print("allocations refused in turn: %r" % counts)
    assert counts == recorded["alloc_walks"]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_pair_refusals.py --record FILE")
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    from pyfeaturetrack_amd.backend import Context
    context = Context(0)
    try:
        record = {"cases": run_cases(context), "alloc_walks": run_walks(context)}
    finally:
        context.close()
    with open(sys.argv[2], "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("recorded %d cases, walks %r" % (len(record["cases"]), record["alloc_walks"]))
