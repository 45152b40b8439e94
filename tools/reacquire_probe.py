#!/usr/bin/env python3
"""Track identities (klt_reacquire_step_async): kernel time of every launch of a step -- the describe launch and the four new ones --
beside the plain tracker launch of the same step, by the dispatches' own timestamps (klt_timing_enable 2), at cfg-2's shape (1080p,
5000 features) and cfg-5's (4K, 20 000).  The pair is a drifting scene whose second frame has a flat block over its middle: the tracks
under it are lost, and as many slots are refilled with features selected on the second frame.  The step is enqueued again and again on
the same list and previous row, so after the warm-up the bank (1024 entries) is full.  For contrast, the same step composed from
klt_match_async on the uncompacted list (a bank's worth of queries against all n descriptors, cross-check on); and KLTTrackSequence's
wall time per frame on a resident clip with the block, with tc.reacquireLost on and off.  Medians of `--reps` calls after `--warmup`.
One JSON line, also written to `--out`.
`python tools/reacquire_probe.py [--reps 15] [--warmup 5] [--out profiles/reacquire_probe.json]`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402
from tools.describe_probe import stats, timed                          # noqa: E402

CAPACITY = 1024
FB_LIST, FB_PREV, FB_CUR = 300, 301, 302


def block(frame):
    h, w = frame.shape
    out = frame.copy()
    out[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = 128
    return out


def shape(cx, res, name, width, height, n, reps, warmup):
    out = res[name] = {"width": width, "height": height, "features": n, "capacity": CAPACITY}
    f1, f2 = synth.synth_pair(width, height, seed=1)
    f2 = block(f2)
    cx.upload(0, f1)
    cx.upload(1, f2)
    cx.build_pyramids_batch([0, 1], sync=True)
    fl, placed = cx.select(0, n, use_pyramid=True)
    tracked, _ = cx.track(0, 1, fl)
    new, _ = cx.select(1, n, use_pyramid=True)
    lost = np.flatnonzero(tracked["val"] < 0)
    step = tracked.copy()
    step[lost] = new[:len(lost)]                             # the lost slots refilled with features of the second frame
    out["placed"], out["lost_tracks"] = int(placed), int(len(lost))
    out["track"] = timed(cx, lambda: cx.track(0, 1, fl), reps, warmup)["track"]
    track_us = out["track"]["median"]
    cx.set_descriptor_params(1)
    cx.set_reacquire_params(capacity=CAPACITY)
    cx.featbuf_upload(FB_LIST, fl)
    cx.reacquire_begin_async(0, FB_LIST, FB_PREV, n)
    cx.featbuf_upload(FB_LIST, step)
    got = timed(cx, lambda: cx.reacquire_step_async(1, FB_LIST, FB_PREV, FB_CUR, n), reps, warmup)
    total = 0.0
    for fam in ("describe", "reacquire_classify", "reacquire_bank", "reacquire_fresh", "reacquire_assign"):
        got[fam]["over_track"] = round(got[fam]["median"] / track_us, 3)
        total += got[fam]["median"]
    out["step"] = {"families": got, "median_sum": round(total, 2), "over_track": round(total / track_us, 3),
                   "new_launches_sum": round(total - got["describe"]["median"], 2)}
    st = cx.reacquire_state()
    out["state_after"] = {k: int(st[k]) for k in st.dtype.names}
    # the same step composed from the entry points that were there: a bank's worth of queries against the uncompacted list
    q, t = cx.describe(0, fl), cx.describe(1, step)
    cx.set_match_params(radius=24)
    m = timed(cx, lambda: cx.match(q[:CAPACITY], t), reps, warmup)
    msum = sum(m[f]["median"] for f in ("match", "match_resolve"))
    out["composed_match_%dx%d" % (CAPACITY, n)] = {"match": m["match"], "match_resolve": m["match_resolve"], "splits": cx.match_path(),
                                                   "median_sum": round(msum, 2), "over_track": round(msum / track_us, 3),
                                                   "over_new_launches": round(msum / max(total - got["describe"]["median"], 1e-9), 2)}
    cx.set_match_params()
    for s in (0, 1):
        cx.slot_free(s)


def sequence(res, name, width, height, n, frames, reps):
    """KLTTrackSequence's wall time per frame on a clip held in host memory, the block over frames 3 .. 7"""
    from pyfeaturetrack_amd import selectGoodFeatures as sgf, trackFeatures as tf
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    sgf.KLT_verbose = tf.KLT_verbose = 0
    base = synth.synth_base(width, height, 17)
    clip = [synth.shift_frame(base, k * 1.0, k * 0.5) for k in range(frames)]
    for k in range(3, 8):
        clip[k] = block(clip[k])
    out = res[name] = {"width": width, "height": height, "features": n, "frames": frames}
    for on in (False, True):
        ms = []
        for r in range(reps + 1):
            tc = KLT_TrackingContext()
            tc.window_width = tc.window_height = 7
            tc.nPyramidLevels, tc.subsampling = 3, 4
            tc.KLTUpdateTCBorder()
            tc.reacquireLost = on
            t0 = time.perf_counter()
            ft = KLTTrackSequence(tc, clip, n)
            if r:
                ms.append((time.perf_counter() - t0) * 1e3 / (frames - 1))
        out["reacquire_on" if on else "reacquire_off"] = dict(stats(ms), unit="ms per frame")
        if on:
            out["reacquired"] = int((ft.ident["val"] == 3).sum())
    out["on_over_off"] = round(out["reacquire_on"]["median"] / out["reacquire_off"]["median"], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reacquire_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    cx.configure(tc)
    res = {"tool": "tools/reacquire_probe.py", "reps": a.reps, "warmup": a.warmup,
           "unit": "microseconds per call, dispatch timestamps (klt_timing_enable 2); sequences: wall milliseconds per frame"}
    shape(cx, res, "cfg2_1080p", 1920, 1080, 5000, a.reps, a.warmup)
    shape(cx, res, "cfg5_4k", 3840, 2160, 20000, a.reps, a.warmup)
    cx.close()
    sequence(res, "sequence_1080p", 1920, 1080, 5000, 24, 5)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
