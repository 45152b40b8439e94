#!/usr/bin/env python3
"""Crowding check (klt_crowd_check_async): kernel time of the check's three launches beside the plain tracker launch of the same list, on
resident frames, alternating in one session: one pair and a batch of `--pairs` pairs at the cfg-2 shape (1080p, 5000 features, d = 10), one
pair at the cfg-5 shape (4K, 20 000 features).  Kernel time by the dispatches' own timestamps (klt_timing_enable 2: the tracker is an
entry of the tracker family, the check's two launches over the records one family, its resolve launch another, their sum is its cost); medians of `--reps` repetitions after
`--warmup`.  The check runs on the tracker's output with ages 0 .. 4 in `prev`, so both of its inputs are read.  Besides: the check's
launches by family (where its time goes), the rounds, and what it flagged.  One JSON line, also written to `--out`.
`python tools/crowd_probe.py [--reps 15] [--warmup 5] [--pairs 8] [--out profiles/crowd_probe.json]`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import CROWD_DTYPE, FEAT_DTYPE, Context      # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

FB_IN, FB_OUT, FB_PREV, FB_CROWD = 100, 200, 300, 400
CHECK = ("crowd_prepare", "crowd_check")      # prepare + rank launches, resolve launch


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def shape(cx, res, name, width, height, n, pairs, reps, warmup, mindist=10):
    cx.set_crowd_params(ncols=width, nrows=height, min_distance=mindist)
    rs = np.random.RandomState(3)
    for p in range(pairs):                                # pair p: slots 2p and 2p + 1, seeds of their own
        f0, f1 = synth.synth_pair(width, height, seed=1 + p)
        for s, f in ((2 * p, f0), (2 * p + 1, f1)):
            cx.upload(s, f)
            cx.build_pyramids(s)
        fl, _ = cx.select(2 * p, n, use_pyramid=True)
        cx.featbuf_upload(FB_IN + p, fl)
        prev = np.zeros(n, CROWD_DTYPE)
        prev["age"] = rs.randint(0, 5, n)
        cx.featbuf_upload(FB_PREV + p, prev.view(FEAT_DTYPE))
    track_pairs = [(2 * p, 2 * p + 1, FB_IN + p, FB_OUT + p) for p in range(pairs)]
    lists = [(FB_OUT + p, FB_PREV + p, FB_CROWD + p) for p in range(pairs)]

    def timed(launch, families):
        cx.timing_enable(2)
        launch()
        cx.sync()
        e = {e["name"]: e for e in cx.timing_read() if e["name"] in families}
        return [e[f]["total_ms"] * 1e3 for f in families], sum(x["launches"] for x in e.values())

    forms = [("single", lambda: cx.track_async(*track_pairs[0], n), lambda: cx.crowd_check_async(*lists[0], n))]
    if pairs > 1:
        forms.append(("batch", lambda: cx.track_batch_async(track_pairs, n), lambda: cx.crowd_check_batch_async(lists, n)))
    out = res[name] = {"width": width, "height": height, "features": n, "min_distance": mindist, "pairs": pairs}
    for form, track, check in forms:
        t_us, c_us, p_us, r_us = [], [], [], []
        for r in range(warmup + reps):                    # alternating: tracker, check, tracker, check, ... (each check on a fresh tracker result)
            t = timed(track, ("track",))[0][0]
            (prepare, resolve), launches = timed(check, CHECK)
            if r >= warmup:
                t_us.append(t)
                c_us.append(prepare + resolve)
                p_us.append(prepare)
                r_us.append(resolve)
        out[form] = {"track_kernel_us": stats(t_us), "crowd_check_kernel_us": stats(c_us), "crowd_check_launches": launches,
                     "prepare_kernel_us": stats(p_us), "resolve_kernel_us": stats(r_us)}
    cx.timing_enable(0)
    # the tracker moves every feature alike on these frames, so its list is as sparse as selection left it: the check's floor.  A list
    # with collisions: every fourth record moved next to its predecessor
    cx.track_async(*track_pairs[0], n)
    cx.crowd_check_async(*lists[0], n)
    rounds, phases = cx.crowd_check_rounds(phases=True)
    out["tracked_list"] = {"rounds": rounds, "resolve_grouping_rounds_records_us": phases, "crowded": int((cx.crowd_download(FB_CROWD, n)["val"] == 2).sum())}
    fl = cx.featbuf_download(FB_OUT, n)
    fl["x"][3::4], fl["y"][3::4] = fl["x"][2:-1:4] + 3, fl["y"][2:-1:4] + 2
    us = []
    for r in range(warmup + reps):
        cx.featbuf_upload(FB_OUT, fl)
        us.append(sum(timed(lambda: cx.crowd_check_async(*lists[0], n), CHECK)[0]))
    cx.timing_enable(0)
    rounds, phases = cx.crowd_check_rounds(phases=True)
    out["colliding_list"] = {"crowd_check_kernel_us": stats(us[warmup:]), "rounds": rounds, "resolve_grouping_rounds_records_us": phases,
                             "crowded": int((cx.crowd_download(FB_CROWD, n)["val"] == 2).sum())}
    for p in range(pairs):
        cx.slot_free(2 * p)
        cx.slot_free(2 * p + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crowd_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    cx.configure(tc)
    res = {"tool": "tools/crowd_probe.py", "reps": a.reps, "warmup": a.warmup}
    shape(cx, res, "cfg2", 1920, 1080, 5000, a.pairs, a.reps, a.warmup)
    shape(cx, res, "cfg5", 3840, 2160, 20000, 1, a.reps, a.warmup)
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
