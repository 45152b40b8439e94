#!/usr/bin/env python3
"""Epipolar check (klt_epipolar_check_async): launch time of the plain tracker, of the motion-model check's three launches and of the
epipolar check's three launches on ONE resident pair of the cfg-2 shape -- 1080p, 5000 features, 7x7, 3 levels, subsampling 4 --,
alternating in one session, and the same for a batch of `--pairs` pairs.  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2; a check's three launches are three entries of the tracker family, their sum is its cost); medians of `--reps`
repetitions after `--warmup`.  Both checks run at their default parameters (256 / 512 hypotheses).  On a tree without the epipolar check
(the parent commit) the tracker and the motion-model check are measured alone.  One JSON line, also written to `--out`.
`python tools/epipolar_probe.py [--reps 15] [--warmup 5] [--pairs 8] [--out profiles/epipolar_probe.json]`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

FB_IN, FB_OUT, FB_M, FB_E = 100, 200, 300, 400


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    n = a.features
    cx = Context(0)
    cx.configure(tc)
    have_check = hasattr(cx, "epipolar_check_async")
    cx.set_model_params(ncols=1920, nrows=1080)
    if have_check:
        cx.set_epipolar_params(ncols=1920, nrows=1080)
    for p in range(a.pairs):                              # pair p: slots 2p and 2p + 1, seeds of their own
        f0, f1 = synth.synth_pair(1920, 1080, seed=1 + p)
        for s, f in ((2 * p, f0), (2 * p + 1, f1)):
            cx.upload(s, f)
            cx.build_pyramids(s)
        fl, _ = cx.select(2 * p, n, use_pyramid=True)
        cx.featbuf_upload(FB_IN + p, fl)
    track_pairs = [(2 * p, 2 * p + 1, FB_IN + p, FB_OUT + p) for p in range(a.pairs)]
    model_pairs = [(FB_IN + p, FB_OUT + p, FB_M + p) for p in range(a.pairs)]
    epi_pairs = [(FB_IN + p, FB_OUT + p, FB_E + p) for p in range(a.pairs)]

    def timed(launch):
        cx.timing_enable(2)
        launch()
        cx.sync()
        e = [e for e in cx.timing_read() if e["name"] == "track"]
        return sum(x["total_ms"] for x in e) * 1e3, sum(x["launches"] for x in e)

    res = {"tool": "tools/epipolar_probe.py", "shape": "cfg2", "features": n, "reps": a.reps, "warmup": a.warmup, "pairs": a.pairs,
           "has_check": have_check}
    forms = (("single", lambda: cx.track_async(*track_pairs[0], n), lambda: cx.motion_check_async(*model_pairs[0], n),
              lambda: cx.epipolar_check_async(*epi_pairs[0], n)),
             ("batch", lambda: cx.track_batch_async(track_pairs, n), lambda: cx.motion_check_batch_async(model_pairs, n),
              lambda: cx.epipolar_check_batch_async(epi_pairs, n)))
    for name, track, model, epipolar in forms:
        t_us, m_us, e_us, launches = [], [], [], 0
        for r in range(a.warmup + a.reps):              # alternating: tracker, motion model, tracker, epipolar, ... (each check on a fresh tracker result)
            t = timed(track)[0]
            m = timed(model)[0]
            e = 0.0
            if have_check:
                timed(track)
                e, launches = timed(epipolar)
            if r >= a.warmup:
                t_us.append(t)
                m_us.append(m)
                e_us.append(e)
        res[name] = {"track_kernel_us": stats(t_us), "model_check_kernel_us": stats(m_us)}
        if have_check:
            res[name]["epipolar_check_kernel_us"] = stats(e_us)
            res[name]["epipolar_check_launches"] = launches
    if have_check:                                        # where the time goes: with ONE hypothesis the scoring launch is next to nothing
        cx.set_epipolar_params(ncols=1920, nrows=1080, hypotheses=1)
        one = []
        for _ in range(a.warmup + a.reps):
            cx.track_async(*track_pairs[0], n)
            one.append(timed(lambda: cx.epipolar_check_async(*epi_pairs[0], n))[0])
        res["single"]["epipolar_check_kernel_us_one_hypothesis"] = stats(one[a.warmup:])
        cx.set_epipolar_params(ncols=1920, nrows=1080)
        cx.track_async(*track_pairs[0], n)
        cx.epipolar_check_async(*epi_pairs[0], n)
    cx.timing_enable(0)
    if have_check:                                      # what the last check of pair 0 left: the tracker's list with the outliers flagged
        out = cx.featbuf_download(FB_OUT, n)
        m = cx.epipolar_download(FB_E)
        res["pair0"] = {"valid": int(m["valid"]), "candidates": int(m["n_candidates"]), "inliers": int(m["n_inliers"]),
                        "flagged": int((out["val"] == -8).sum())}
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
