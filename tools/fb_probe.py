#!/usr/bin/env python3
"""Forward-backward check: the fused call (klt_track_fb*) against the composition a caller has to build without it -- klt_track_async twice
on the plain kernels (1 -> 2, then 2 -> 1 on the result) plus the rule on the host -- on the 8-pair batched cfg-2 shape (1080p, 5000
features, 7x7, 3 levels, subsampling 4), the single cfg-2 pair and cfg-3 (15x15, 4 levels).  Kernel time by the dispatches' own timestamps
(klt_timing_enable 2), wall-clock time around the whole call up to the records on the host.  Medians of `--reps` repetitions after
`--warmup`; writes profiles/fb_probe.json.  `python tools/fb_probe.py [--reps 9] [--warmup 3] [--out profiles/fb_probe.json]`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402


def make_tc(levels, ss, window):
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = window
    tc.nPyramidLevels, tc.subsampling = levels, ss
    tc.KLTUpdateTCBorder()
    return tc


def host_rule(fin, fwd, back, max_error):
    out = fwd.copy()
    checked = (fin["val"] >= 0) & (fwd["val"] == 0)
    dx = (back["x"] - fin["x"]).astype(np.float64)
    dy = (back["y"] - fin["y"]).astype(np.float64)
    ok = (back["val"] == 0) & (dx * dx + dy * dy <= float(np.float32(max_error)) ** 2)
    rej = checked & ~ok
    out["x"][rej] = -1.0
    out["y"][rej] = -1.0
    out["val"][rej] = -6
    return out


def track_ms(cx):
    return sum(e["total_ms"] for e in cx.timing_read() if e["name"] == "track")


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def probe(cx, name, tc, frames, n, npairs, reps, warmup, max_error=1.0):
    cx.configure(tc)
    cx.set_fb_params(max_error=max_error)
    pairs = []
    for i in range(npairs):
        f0, f1 = frames(i)
        s0, s1 = 2 * i, 2 * i + 1
        cx.upload(s0, f0)
        cx.upload(s1, f1)
        cx.build_pyramids(s0)
        cx.build_pyramids(s1)
        fl, _ = cx.select(s0, n, use_pyramid=True)
        cx.featbuf_upload(100 + i, fl)
        pairs.append((s0, s1, fl))
    fin = [p[2] for p in pairs]

    def fused():
        if npairs == 1:
            cx.track_fb_async(0, 1, 100, 200, n)
        else:
            cx.track_fb_batch_async([(2 * i, 2 * i + 1, 100 + i, 200 + i) for i in range(npairs)], n)
        cx.sync()
        return [cx.featbuf_download(200 + i, n) for i in range(npairs)]

    def composed():
        if npairs == 1:
            cx.track_async(0, 1, 100, 300, n)
            cx.track_async(1, 0, 300, 400, n)
        else:
            cx.track_batch_async([(2 * i, 2 * i + 1, 100 + i, 300 + i) for i in range(npairs)], n)
            cx.track_batch_async([(2 * i + 1, 2 * i, 300 + i, 400 + i) for i in range(npairs)], n)
        cx.sync()
        out = []
        for i in range(npairs):
            fwd, back = cx.featbuf_download(300 + i, n), cx.featbuf_download(400 + i, n)
            out.append(host_rule(fin[i], fwd, back, max_error))
        return out

    res = {"shape": name, "pairs": npairs, "features": n, "window": tc.window_width, "levels": tc.nPyramidLevels}
    outs = {}
    for label, fn in (("composition", composed), ("fused", fused), ("composition_again", composed)):
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
    same = all(np.array_equal(a[k], b[k]) for a, b in zip(outs["fused"], outs["composition"]) for k in ("x", "y", "val", "aux"))
    res["records_identical"] = bool(same)
    res["rejected"] = int(sum((o["val"] == -6).sum() for o in outs["fused"]))
    comp = [res["composition"], res["composition_again"]]
    for what in ("kernel_ms", "wall_ms"):
        base = min(c[what]["median"] for c in comp)
        res["ratio_" + what] = res["fused"][what]["median"] / base
        res["composition_spread_" + what] = max(c[what]["max"] for c in comp) / min(c[what]["min"] for c in comp)
    for s in range(2 * npairs):
        cx.slot_free(s)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fb_probe.json"))
    a = ap.parse_args()
    cx = Context(0)
    results = []

    def occluded(width, height, seed, shift):
        base = synth.synth_base(width, height, seed)
        f0, f1 = synth.shift_frame(base, 0.0, 0.0), synth.shift_frame(base, shift[0], shift[1])
        f1[height // 4:height // 2, width // 4:width // 2] = f0[0:height // 4, 0:width // 4]      # something for the check to reject
        return f0, f1

    cfg2 = {}

    def cfg2_frames(i):
        if i not in cfg2:
            cfg2[i] = occluded(1920, 1080, 1 + i, synth.DEFAULT_SHIFT)
        return cfg2[i]

    results.append(probe(cx, "cfg2_batch8", make_tc(3, 4, 7), cfg2_frames, 5000, 8, a.reps, a.warmup))
    results.append(probe(cx, "cfg2_single", make_tc(3, 4, 7), cfg2_frames, 5000, 1, a.reps, a.warmup))
    cfg3 = occluded(1920, 1080, 1, (1.1, -0.7))
    results.append(probe(cx, "cfg3", make_tc(4, 2, 15), lambda i: cfg3, 5000, 1, a.reps, a.warmup))
    cx.close()
    for r in results:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/fb_probe.py", "reps": a.reps, "warmup": a.warmup, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
