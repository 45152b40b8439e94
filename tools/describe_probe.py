#!/usr/bin/env python3
"""Descriptors and their matcher (klt_describe_async, klt_match_async): kernel time of the describe launch (both modes) and of the match
launches beside the plain tracker launch and the selection of the same shape, by the dispatches' own timestamps where a family is one
launch (klt_timing_enable 2: describe, match, match_resolve, track; the selection is the sum of its families, some of them event pairs).
Two shapes: cfg-2's (1080p, 5000 features: 5000 x 5000 and 300 x 5000 matches) and cfg-5's (4K, 20 000 features: 20 000 x 20 000 and
300 x 20 000).  The train set of a match is the frame-2 descriptors of the tracked list, the query set the frame-1 descriptors (or their
first 300): real descriptors, with the default parameters (cross-check on: two match launches and the resolve launch).  Medians of
`--reps` calls after `--warmup`.  One JSON line, also written to `--out`.
`python tools/describe_probe.py [--reps 15] [--warmup 5] [--out profiles/describe_probe.json]`."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def timed(cx, call, reps, warmup):
    """microseconds per call of every kernel family `call` launches: {family: stats}, and the launches per call"""
    us, launches = {}, {}
    for r in range(warmup + reps):
        cx.timing_enable(2)
        call()
        cx.sync()
        entries = [e for e in cx.timing_read() if "!" not in e["name"]]
        cx.timing_enable(0)
        if r >= warmup:
            for e in entries:
                us.setdefault(e["name"], []).append(e["total_ms"] * 1e3)
                launches[e["name"]] = e["launches"]
    return {f: dict(stats(v), launches=launches[f]) for f, v in us.items()}


def shape(cx, res, name, width, height, n, reps, warmup):
    out = res[name] = {"width": width, "height": height, "features": n}
    f1, f2 = synth.synth_pair(width, height, seed=1)
    cx.upload(0, f1)
    cx.upload(1, f2)
    cx.build_pyramids_batch([0, 1], sync=True)
    fl, placed = cx.select(0, n, use_pyramid=True)
    tracked, _ = cx.track(0, 1, fl)
    out["placed"] = int(placed)
    out["track"] = timed(cx, lambda: cx.track(0, 1, fl), reps, warmup)["track"]
    sel = timed(cx, lambda: cx.select(0, n, use_pyramid=True), reps, warmup)
    out["select"] = {"families": sel, "median_sum": round(sum(v["median"] for v in sel.values()), 2)}
    track_us = out["track"]["median"]
    desc = {}
    for mode, label in ((1, "upright"), (2, "steered")):
        cx.set_descriptor_params(mode)
        got = out["describe_" + label] = timed(cx, lambda: cx.describe(0, fl), reps, warmup)["describe"]
        got["over_track"] = round(got["median"] / track_us, 3)
        got["ns_per_feature"] = round(got["median"] * 1e3 / n, 1)
        desc[mode] = (cx.describe(0, fl), cx.describe(1, tracked))
    cx.set_match_params()
    q, t = desc[1]
    for nq in (n, 300):
        got = timed(cx, lambda: cx.match(q[:nq], t), reps, warmup)
        total = sum(got[f]["median"] for f in ("match", "match_resolve"))
        out["match_%dx%d" % (nq, n)] = {"match": got["match"], "match_resolve": got["match_resolve"], "splits": cx.match_path(),
                                        "median_sum": round(total, 2), "over_track": round(total / track_us, 3),
                                        "pairs_per_ns": round(2.0 * nq * n / (got["match"]["median"] * 1e3), 2)}
    for s in (0, 1):
        cx.slot_free(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    cx.configure(tc)
    res = {"tool": "tools/describe_probe.py", "reps": a.reps, "warmup": a.warmup,
           "unit": "microseconds per call, dispatch timestamps (klt_timing_enable 2); match: the forward and the backward launch together"}
    shape(cx, res, "cfg2_1080p", 1920, 1080, 5000, a.reps, a.warmup)
    shape(cx, res, "cfg5_4k", 3840, 2160, 20000, a.reps, a.warmup)
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
