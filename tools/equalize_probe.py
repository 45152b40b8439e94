#!/usr/bin/env python3
"""CLAHE ingest stage (klt_set_equalize_params): kernel time of its two launches beside the level-0 launch of the same build, by the
dispatches' own timestamps (klt_timing_enable 2: clahe_lut_kernel is the family equalize_lut, clahe_apply_kernel equalize_apply, the
level-0 launch smooth_grad_l0).  At 1080p and at 4K, for one frame and for a batch of `--batch` frames in one build, on a random frame
(the texture of the benchmark) and on a constant frame -- the frame on which every pixel of a tile falls into one histogram bin.  Every
build is of freshly uploaded frames, so every build equalises; 8 x 8 tiles, clip limit 3.0; medians of `--reps` builds after `--warmup`.
Besides, per shape: the ratio of the two launches to the level-0 launch and of clahe_lut_kernel's time on the constant frame to its time
on the random one.  One JSON line, also written to `--out`.
`python tools/equalize_probe.py [--reps 15] [--warmup 5] [--batch 16] [--out profiles/equalize_probe.json]`."""
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

FAMILIES = ("equalize_lut", "equalize_apply", "smooth_grad_l0")


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def builds(cx, frames, reps, warmup):
    """microseconds per build of each family: `frames` uploaded into slots 0 .. and built in one call, again and again"""
    slots = list(range(len(frames)))
    us = {f: [] for f in FAMILIES}
    for r in range(warmup + reps):
        for s, f in zip(slots, frames):
            cx.upload(s, f)
        cx.timing_enable(2)
        cx.build_pyramids_batch(slots, sync=True)
        e = {e["name"]: e for e in cx.timing_read()}
        cx.timing_enable(0)
        assert cx.equalize_path() == 1 and all(e[f]["launches"] == 1 for f in FAMILIES), e
        if r >= warmup:
            for f in FAMILIES:
                us[f].append(e[f]["total_ms"] * 1e3)
    return {f: stats(v) for f, v in us.items()}


def shape(cx, res, name, width, height, batch, reps, warmup):
    out = res[name] = {"width": width, "height": height}
    random = [synth.synth_pair(width, height, seed=1 + k)[0] for k in range(2)]
    constant = np.full((height, width), 77, np.uint8)
    for count in (1, batch):
        form = out["frames_%d" % count] = {}
        for kind, frames in (("random", [random[k % 2] for k in range(count)]), ("constant", [constant] * count)):
            form[kind] = builds(cx, frames, reps, warmup)
        r, c = form["random"], form["constant"]
        form["equalize_over_level0_random"] = round((r["equalize_lut"]["median"] + r["equalize_apply"]["median"]) / r["smooth_grad_l0"]["median"], 3)
        form["lut_constant_over_random"] = round(c["equalize_lut"]["median"] / r["equalize_lut"]["median"], 3)
    for s in range(batch):
        cx.slot_free(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "equalize_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    cx.configure(tc)
    cx.set_equalize_params(mode=1, tiles_x=8, tiles_y=8, clip_q8=768)
    res = {"tool": "tools/equalize_probe.py", "reps": a.reps, "warmup": a.warmup, "batch": a.batch, "tiles": [8, 8], "clip_limit": 3.0,
           "unit": "microseconds per launch, dispatch timestamps"}
    shape(cx, res, "1080p", 1920, 1080, a.batch, a.reps, a.warmup)
    shape(cx, res, "4k", 3840, 2160, a.batch, a.reps, a.warmup)
    cx.close()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
