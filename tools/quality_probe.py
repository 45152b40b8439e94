#!/usr/bin/env python3
"""Track quality (klt_track_quality_async): launch time of the plain tracker and of the quality launch on ONE resident pair of the cfg-2
shape -- 1080p, 5000 features, 7x7, 3 levels, subsampling 4 -- alternating in one session.  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2); medians of `--reps` repetitions after `--warmup`.  The quality launch reads the list the tracker read and the one
it wrote.  One JSON line, also written to `--out`; "quality_faster" is the condition of DESIGN.md section 9f.
`python tools/quality_probe.py [--reps 15] [--warmup 5] [--out profiles/quality_probe.json]`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

FB_IN, FB_OUT, FB_Q = 100, 200, 300


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--window", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = a.window
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    n = a.features
    cx = Context(0)
    cx.configure(tc)
    f0, f1 = synth.synth_pair(1920, 1080, seed=1)
    for s, f in ((0, f0), (1, f1)):
        cx.upload(s, f)
        cx.build_pyramids(s)
    fl, _ = cx.select(0, n, use_pyramid=True)
    cx.featbuf_upload(FB_IN, fl)

    def timed(launch):
        cx.timing_enable(2)
        launch()
        cx.sync()
        return sum(e["total_ms"] for e in cx.timing_read() if e["name"] == "track") * 1e3

    track, quality = [], []
    for r in range(a.warmup + a.reps):                  # alternating: tracker, quality, tracker, ...
        t = timed(lambda: cx.track_async(0, 1, FB_IN, FB_OUT, n))
        q = timed(lambda: cx.track_quality_async(0, 1, FB_IN, FB_OUT, FB_Q, n))
        if r >= a.warmup:
            track.append(t)
            quality.append(q)
    cx.timing_enable(0)
    out = cx.featbuf_download(FB_OUT, n)
    rec = cx.quality_download(FB_Q, n)
    res = {"tool": "tools/quality_probe.py", "shape": "cfg2_single", "features": n, "window": a.window, "reps": a.reps, "warmup": a.warmup,
           "track": {"kernel_us": stats(track), "tracked": int((out["val"][fl["val"] >= 0] == 0).sum())},
           "quality": {"kernel_us": stats(quality), "measured": int((rec["val"] == 1).sum())}}
    res["quality_faster"] = bool(res["quality"]["kernel_us"]["median"] < res["track"]["kernel_us"]["median"])
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
