#!/usr/bin/env python3
"""Homography check (klt_homography_check_async): launch time of the plain tracker and of the three launches of each consensus check --
motion model, epipolar, homography -- on ONE resident pair of the cfg-2 shape -- 1080p, 5000 features, 7x7, 3 levels, subsampling 4 --,
alternating in one session, and the same for a batch of `--pairs` pairs.  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2; a check's three launches are three entries of the tracker family, their sum is its cost); medians of `--reps`
repetitions after `--warmup`.  Every check runs at its default parameters (256 / 512 / 256 hypotheses); the epipolar check is the
yardstick: the same launch shape, the same three null9 on the critical path.  On a tree without the homography check (the parent commit)
the tracker and the other two checks are measured alone.  One JSON line, also written to `--out`.
`python tools/homography_probe.py [--reps 15] [--warmup 5] [--pairs 8] [--out profiles/homography_probe.json]`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

FB_IN, FB_OUT, FB_M, FB_E, FB_H = 100, 200, 300, 400, 500


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    n = a.features
    cx = Context(0)
    cx.configure(tc)
    have_check = hasattr(cx, "homography_check_async")
    cx.set_model_params(ncols=1920, nrows=1080)
    cx.set_epipolar_params(ncols=1920, nrows=1080)
    if have_check:
        cx.set_homography_params(ncols=1920, nrows=1080)
    for p in range(a.pairs):                              # pair p: slots 2p and 2p + 1, seeds of their own
        f0, f1 = synth.synth_pair(1920, 1080, seed=1 + p)
        for s, f in ((2 * p, f0), (2 * p + 1, f1)):
            cx.upload(s, f)
            cx.build_pyramids(s)
        fl, _ = cx.select(2 * p, n, use_pyramid=True)
        cx.featbuf_upload(FB_IN + p, fl)
    track_pairs = [(2 * p, 2 * p + 1, FB_IN + p, FB_OUT + p) for p in range(a.pairs)]
    pairs_of = {name: [(FB_IN + p, FB_OUT + p, fb + p) for p in range(a.pairs)] for name, fb in (("model", FB_M), ("epipolar", FB_E),
                                                                                                 ("homography", FB_H))}

    def timed(launch):
        cx.timing_enable(2)
        launch()
        cx.sync()
        e = [e for e in cx.timing_read() if e["name"] == "track"]
        return sum(x["total_ms"] for x in e) * 1e3, sum(x["launches"] for x in e)

    res = {"tool": "tools/homography_probe.py", "shape": "cfg2", "features": n, "reps": a.reps, "warmup": a.warmup, "pairs": a.pairs,
           "has_check": have_check}
    single = {"model": lambda: cx.motion_check_async(*pairs_of["model"][0], n), "epipolar": lambda: cx.epipolar_check_async(*pairs_of["epipolar"][0], n)}
    batch = {"model": lambda: cx.motion_check_batch_async(pairs_of["model"], n), "epipolar": lambda: cx.epipolar_check_batch_async(pairs_of["epipolar"], n)}
    if have_check:
        single["homography"] = lambda: cx.homography_check_async(*pairs_of["homography"][0], n)
        batch["homography"] = lambda: cx.homography_check_batch_async(pairs_of["homography"], n)
    forms = (("single", lambda: cx.track_async(*track_pairs[0], n), single), ("batch", lambda: cx.track_batch_async(track_pairs, n), batch))
    for name, track, checks in forms:
        us = {k: [] for k in ["track"] + list(checks)}
        launches = {}
        for r in range(a.warmup + a.reps):              # alternating: tracker, check, tracker, check, ... (each check on a fresh tracker result)
            for k, check in checks.items():
                t = timed(track)[0]
                c, launches[k] = timed(check)
                if r >= a.warmup:
                    us["track"].append(t)
                    us[k].append(c)
        res[name] = {"track_kernel_us": stats(us["track"])}
        for k in checks:
            res[name][k + "_check_kernel_us"] = stats(us[k])
            res[name][k + "_check_launches"] = launches[k]
    if have_check:                                        # where the time goes: with ONE hypothesis the scoring launch is next to nothing
        cx.set_homography_params(ncols=1920, nrows=1080, hypotheses=1)
        one = []
        for _ in range(a.warmup + a.reps):
            cx.track_async(*track_pairs[0], n)
            one.append(timed(lambda: cx.homography_check_async(*pairs_of["homography"][0], n))[0])
        res["single"]["homography_check_kernel_us_one_hypothesis"] = stats(one[a.warmup:])
        cx.set_homography_params(ncols=1920, nrows=1080)
        cx.track_async(*track_pairs[0], n)
        cx.homography_check_async(*pairs_of["homography"][0], n)
    cx.timing_enable(0)
    if have_check:                                      # what the last check of pair 0 left: the tracker's list with the outliers flagged
        out = cx.featbuf_download(FB_OUT, n)
        m = cx.homography_download(FB_H)
        res["pair0"] = {"valid": int(m["valid"]), "candidates": int(m["n_candidates"]), "inliers": int(m["n_inliers"]),
                        "flagged": int((out["val"] == -9).sum())}
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
