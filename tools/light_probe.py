#!/usr/bin/env python3
"""Gain / bias tracking (klt_set_light_params mode 1): launch time of the plain tracker, of the lighting wave kernel (one feature per
wavefront; KLT_OPT_TRACK_VARIANT 0) and of the lighting quad kernel (four 7x7 features per wavefront) on ONE resident pair of the cfg-2
shape -- 1080p, 5000 features, 7x7, 3 levels, subsampling 4.  Kernel time by the dispatches' own timestamps (klt_timing_enable 2); the
plain tracker is measured before and after the lighting launches, for its own spread.  Medians of `--reps` repetitions after `--warmup`;
one JSON line, also written to `--out`.  `python tools/light_probe.py [--reps 15] [--warmup 5] [--out profiles/light_probe.json]`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyfeaturetrack_amd import synth                                   # noqa: E402
from pyfeaturetrack_amd.backend import Context                         # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                 # noqa: E402

OPT_TRACK_VARIANT = 11


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    n = a.features
    cx = Context(0)
    has_light = hasattr(cx, "set_light_params")            # (the same script measures the plain tracker of a tree without the feature)
    cx.configure(tc)
    f0, f1 = synth.synth_pair(1920, 1080, seed=1)
    f1 = np.clip(np.floor(0.7 * f1.astype(np.float64) + 40.0 + 0.5), 0, 255).astype(np.uint8)      # a gain and an offset on frame 2
    for s, f in ((0, f0), (1, f1)):
        cx.upload(s, f)
        cx.build_pyramids(s)
    fl, _ = cx.select(0, n, use_pyramid=True)
    cx.featbuf_upload(100, fl)

    def measure(label, path):
        kern = []
        for r in range(a.warmup + a.reps):
            cx.timing_enable(2)
            cx.track_async(0, 1, 100, 200, n)
            cx.sync()
            k = sum(e["total_ms"] for e in cx.timing_read() if e["name"] == "track")
            if r >= a.warmup:
                kern.append(k * 1e3)
        cx.timing_enable(0)
        if path is not None:
            assert cx.track_light_path() == path, (label, cx.track_light_path())
        out = cx.featbuf_download(200, n)
        return {"kernel_us": stats(kern), "tracked": int((out["val"][fl["val"] >= 0] == 0).sum())}, out

    res = {"tool": "tools/light_probe.py", "shape": "cfg2_single", "features": n, "reps": a.reps, "warmup": a.warmup}
    res["plain"], _ = measure("plain", None)
    if has_light:
        try:
            cx.set_light_params(mode=1)
            res["light_quad"], quad = measure("light_quad", 2)
            cx.set_option(OPT_TRACK_VARIANT, 0)
            res["light_wave"], wave = measure("light_wave", 1)
            res["records_identical"] = bool(all(np.array_equal(quad[k], wave[k]) for k in ("x", "y", "val", "aux")))
        finally:
            cx.set_option(OPT_TRACK_VARIANT, 4)
            cx.set_light_params(mode=0)
    res["plain_again"], _ = measure("plain_again", None)
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
