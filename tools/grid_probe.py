#!/usr/bin/env python3
"""Selection grid (klt_set_select_grid): what the per-cell quota costs, per timing family of the library (klt_timing_enable 1).

Shape a: 1080p, 5000 features, 3 levels, subsampling 4 -- KLT_SELECTING_ALL and a KLT_REPLACING_SOME with about 2 % of the features lost,
each without a grid and under 120x120 / 60 and 240x270 / 200.  Shape b: 4K, 20 000 features, a replacement with 80 features lost -- how
often klt_select_finish reports a rewritten list (a repeat), without a grid and under two grids, for the candidate cut as it is and widened
(KLT_GRID_CUT_SCALE, read by the library when it plans a selection under a grid).  Shape w: the frame of shape a, KLT_SELECTING_ALL -- the
greedy walk (KLT_OPT_SELECT_PARALLEL_NMS = 0) without a grid and under 120x120 / 4, and the default path (filter + placement by rank) under
that grid.  Medians of `--reps` selections after `--warmup`.
`--root DIR` measures another checkout of the project (one without the feature runs the legs without a grid only), so that two trees can
be alternated in one session:  python tools/grid_probe.py [--shape a|b|w] [--root DIR] [--cut-scale K] [--reps 15] [--warmup 5] [--out F]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECTING_ALL, REPLACING_SOME = 1, 2
KLT_OPT_SELECT_PARALLEL_NMS = 8
FB = 120


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def lose(fl, count, seed):
    out = fl.copy()
    lost = np.random.default_rng(seed).choice(len(out), count, replace=False)
    out["x"][lost], out["y"][lost], out["val"][lost] = -1.0, -1.0, -1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="a", choices=["a", "b", "w"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--cut-scale", type=int, default=0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cut_scale:
        os.environ["KLT_GRID_CUT_SCALE"] = str(a.cut_scale)
    sys.path.insert(0, os.path.abspath(a.root))
    from pyfeaturetrack_amd import synth
    from pyfeaturetrack_amd.backend import Context
    from pyfeaturetrack_amd.klt import KLT_TrackingContext

    tc = KLT_TrackingContext()
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    has_grid = hasattr(cx, "set_select_grid")
    cx.configure(tc)
    walks = [False]                                               # per leg: the greedy walk in place of the parallel passes
    if a.shape in "aw":
        img, n, lost = synth.synth_pair(1920, 1080, seed=1)[0], 5000, 100
        grids = [None, (120, 120, 60), (240, 270, 200)]
        modes = [SELECTING_ALL, REPLACING_SOME]
        if a.shape == "w":
            grids, modes, walks = [None, (120, 120, 4)], [SELECTING_ALL], [True, False]
    else:
        img, n, lost = synth.shift_frame(synth.synth_base(3840, 2160, 4), 0.0, 0.0), 20000, 80
        grids = [None, (120, 120, 60), (240, 270, 40)]
        modes = [REPLACING_SOME]
    cx.upload(0, img)
    cx.build_pyramids(0, sync=True)
    plain = cx.select(0, n, use_pyramid=True)[0]
    start = lose(plain, lost, 7)

    def leg(mode, grid, walk=False):
        if grid is not None:
            cx.set_select_grid(grid)
        cx.set_option(KLT_OPT_SELECT_PARALLEL_NMS, 0 if walk else 1)
        fams, wall, repeats = {}, [], 0
        for r in range(a.warmup + a.reps):
            cx.featbuf_upload(FB, start if mode == REPLACING_SOME else plain)
            cx.sync()
            cx.timing_enable(1)
            t0 = time.perf_counter()
            cx.select_begin(0, mode, True, FB, n)
            again = cx.select_finish()
            cx.sync()
            t1 = time.perf_counter()
            read = cx.timing_read()
            cx.timing_enable(0)
            if r < a.warmup:
                continue
            repeats += bool(again)
            wall.append((t1 - t0) * 1e3)
            for e in read:
                if e["launches"]:
                    fams.setdefault(e["name"], []).append(e["total_ms"])
            fams.setdefault("all_families", []).append(sum(e["total_ms"] for e in read))
        got = cx.featbuf_download(FB, n)
        free = np.ones(n, bool) if mode == SELECTING_ALL else start["val"] < 0
        out = {"families_ms": {k: round(median(v), 5) for k, v in sorted(fams.items())}, "wall_ms": round(median(wall), 5),
               "wall_ms_min_max": [round(min(wall), 5), round(max(wall), 5)], "repeats": repeats, "reps": a.reps,
               "filled": int((got["val"][free] >= 0).sum()), "free": int(free.sum())}
        if grid is not None:
            out["grid_path"] = cx.select_grid_path()
            cx.set_select_grid(None)
        return out

    res = {"tool": "tools/grid_probe.py", "label": a.label, "shape": a.shape, "features": n, "lost": lost, "reps": a.reps,
           "warmup": a.warmup, "cut_scale": a.cut_scale or 1, "has_grid": has_grid, "legs": {}}
    for walk in walks:
        for mode in modes:
            for grid in grids:
                if grid is not None and not has_grid:
                    continue
                name = "%s%s/%s" % ("walk " if walk else "", "all" if mode == SELECTING_ALL else "replace", "none" if grid is None else "%dx%d/%d" % grid)
                res["legs"][name] = leg(mode, grid, walk)
    # once more without a grid: the spread of the figures that must not move
    for mode in modes:
        res["legs"]["%s%s/none again" % ("walk " if walks[0] else "", "all" if mode == SELECTING_ALL else "replace")] = leg(mode, None, walks[0])
    cx.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
