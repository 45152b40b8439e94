#!/usr/bin/env python3
"""Motion prior: klt_track_guess_async with an identity guess (the list is its own guess list: the same work as the plain call plus one
16-byte record load per feature) against klt_track_async of the same build -- on the single cfg-2 pair (1080p, 5000 features, 7x7, 3
levels, subsampling 4), the 8-pair batched cfg-2 shape and cfg-3's window (15x15, 4 levels).  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2).  The plain call is measured before and after the guess call, for its own spread.  Medians of `--reps` repetitions
after `--warmup`; writes profiles/guess_probe.json.  `python tools/guess_probe.py [--reps 9] [--warmup 3] [--out profiles/guess_probe.json]`."""
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


def make_tc(levels, ss, window):
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = window
    tc.nPyramidLevels, tc.subsampling = levels, ss
    tc.KLTUpdateTCBorder()
    return tc


def track_ms(cx):
    return sum(e["total_ms"] for e in cx.timing_read() if e["name"] == "track")


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def probe(cx, name, tc, frames, n, npairs, reps, warmup):
    cx.configure(tc)
    for i in range(npairs):
        f0, f1 = frames(i)
        s0, s1 = 2 * i, 2 * i + 1
        cx.upload(s0, f0)
        cx.upload(s1, f1)
        cx.build_pyramids(s0)
        cx.build_pyramids(s1)
        fl, _ = cx.select(s0, n, use_pyramid=True)
        cx.featbuf_upload(100 + i, fl)

    def plain():
        if npairs == 1:
            cx.track_async(0, 1, 100, 200, n)
        else:
            cx.track_batch_async([(2 * i, 2 * i + 1, 100 + i, 200 + i) for i in range(npairs)], n)
        cx.sync()
        return [cx.featbuf_download(200 + i, n) for i in range(npairs)]

    def guess():
        if npairs == 1:
            cx.track_guess_async(0, 1, 100, 100, 300, n)
        else:
            cx.track_guess_batch_async([(2 * i, 2 * i + 1, 100 + i, 100 + i, 300 + i) for i in range(npairs)], n)
        cx.sync()
        return [cx.featbuf_download(300 + i, n) for i in range(npairs)]

    res = {"shape": name, "pairs": npairs, "features": n, "window": tc.window_width, "levels": tc.nPyramidLevels}
    outs = {}
    for label, fn in (("plain", plain), ("guess", guess), ("plain_again", plain)):
        wall, kern = [], []
        for r in range(warmup + reps):
            cx.timing_enable(2)
            t0 = time.perf_counter()
            o = fn()
            t1 = time.perf_counter()
            k = track_ms(cx)
            if r >= warmup:
                wall.append((t1 - t0) * 1e3)
                kern.append(k)
        cx.timing_enable(0)
        outs[label] = o
        res[label] = {"kernel_ms": stats(kern), "wall_ms": stats(wall)}
    res["records_identical"] = bool(all(np.array_equal(a[k], b[k]) for a, b in zip(outs["guess"], outs["plain"])
                                        for k in ("x", "y", "val", "aux")))
    both = [res["plain"], res["plain_again"]]
    for what in ("kernel_ms", "wall_ms"):
        res["ratio_" + what] = res["guess"][what]["median"] / min(c[what]["median"] for c in both)
        res["plain_spread_" + what] = max(c[what]["max"] for c in both) / min(c[what]["min"] for c in both)
    for s in range(2 * npairs):
        cx.slot_free(s)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guess_probe.json"))
    a = ap.parse_args()
    cx = Context(0)
    results = []
    cfg2 = {}

    def cfg2_frames(i):
        if i not in cfg2:
            cfg2[i] = synth.synth_pair(1920, 1080, seed=1 + i)
        return cfg2[i]

    results.append(probe(cx, "cfg2_single", make_tc(3, 4, 7), cfg2_frames, 5000, 1, a.reps, a.warmup))
    results.append(probe(cx, "cfg2_batch8", make_tc(3, 4, 7), cfg2_frames, 5000, 8, a.reps, a.warmup))
    base = synth.synth_base(1920, 1080, 1)
    cfg3 = [synth.synth_frame(1920, 1080, 1, k, shift=(1.1, -0.7), base=base) for k in range(2)]
    results.append(probe(cx, "cfg3", make_tc(4, 2, 15), lambda i: cfg3, 5000, 1, a.reps, a.warmup))
    cx.close()
    for r in results:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/guess_probe.py", "reps": a.reps, "warmup": a.warmup, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
