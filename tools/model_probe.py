#!/usr/bin/env python3
"""Motion-model check (klt_motion_check_async): launch time of the plain tracker and of the check's three launches on ONE resident pair of
the cfg-2 shape -- 1080p, 5000 features, 7x7, 3 levels, subsampling 4 --, alternating in one session, and the same for a batch of
`--pairs` pairs (klt_track_batch_async against klt_motion_check_batch_async).  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2; the check's three launches are three entries of the tracker family, their sum is its cost); medians of `--reps`
repetitions after `--warmup`.  On a tree without the check (the parent commit) only the tracker is measured.  One JSON line, also written
to `--out`; "check_cheaper" is the condition of DESIGN.md section 9g.
`python tools/model_probe.py [--reps 15] [--warmup 5] [--pairs 8] [--hypotheses 256] [--out profiles/model_probe.json]`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

FB_IN, FB_OUT, FB_M = 100, 200, 300


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    n = a.features
    cx = Context(0)
    cx.configure(tc)
    have_check = hasattr(cx, "motion_check_async")
    if have_check:
        cx.set_model_params(ncols=1920, nrows=1080, hypotheses=a.hypotheses)
    for p in range(a.pairs):                              # pair p: slots 2p and 2p + 1, seeds of their own
        f0, f1 = synth.synth_pair(1920, 1080, seed=1 + p)
        for s, f in ((2 * p, f0), (2 * p + 1, f1)):
            cx.upload(s, f)
            cx.build_pyramids(s)
        fl, _ = cx.select(2 * p, n, use_pyramid=True)
        cx.featbuf_upload(FB_IN + p, fl)
    track_pairs = [(2 * p, 2 * p + 1, FB_IN + p, FB_OUT + p) for p in range(a.pairs)]
    check_pairs = [(FB_IN + p, FB_OUT + p, FB_M + p) for p in range(a.pairs)]

    def timed(launch):
        cx.timing_enable(2)
        launch()
        cx.sync()
        e = [e for e in cx.timing_read() if e["name"] == "track"]
        return sum(x["total_ms"] for x in e) * 1e3, sum(x["launches"] for x in e)

    res = {"tool": "tools/model_probe.py", "shape": "cfg2", "features": n, "hypotheses": a.hypotheses, "reps": a.reps, "warmup": a.warmup,
           "pairs": a.pairs, "has_check": have_check}
    for name, track, check in (("single", lambda: cx.track_async(*track_pairs[0], n), lambda: cx.motion_check_async(*check_pairs[0], n)),
                               ("batch", lambda: cx.track_batch_async(track_pairs, n), lambda: cx.motion_check_batch_async(check_pairs, n))):
        t_us, c_us, launches = [], [], 0
        for r in range(a.warmup + a.reps):              # alternating: tracker, check, tracker, ...
            t = timed(track)[0]
            c, launches = timed(check) if have_check else (0.0, 0)
            if r >= a.warmup:
                t_us.append(t)
                c_us.append(c)
        res[name] = {"track_kernel_us": stats(t_us)}
        if have_check:
            res[name]["check_kernel_us"] = stats(c_us)
            res[name]["check_launches"] = launches
            res[name]["check_cheaper"] = bool(stats(c_us)["median"] < stats(t_us)["median"])
    if have_check:                                        # where the time goes: with ONE hypothesis the scoring launch is next to nothing
        cx.set_model_params(ncols=1920, nrows=1080, hypotheses=1)
        one = [timed(lambda: cx.motion_check_async(*check_pairs[0], n))[0] for _ in range(a.warmup + a.reps)][a.warmup:]
        res["single"]["check_kernel_us_one_hypothesis"] = stats(one)
        cx.set_model_params(ncols=1920, nrows=1080, hypotheses=a.hypotheses)
        cx.track_async(*track_pairs[0], n)
        cx.motion_check_async(*check_pairs[0], n)
    cx.timing_enable(0)
    if have_check:                                      # what the last check of pair 0 left: the tracker's list with the outliers flagged
        out = cx.featbuf_download(FB_OUT, n)
        m = cx.model_download(FB_M)
        res["pair0"] = {"valid": int(m["valid"]), "candidates": int(m["n_candidates"]), "inliers": int(m["n_inliers"]),
                        "flagged": int((out["val"] == -7).sum())}
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
