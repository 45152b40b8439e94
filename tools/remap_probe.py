#!/usr/bin/env python3
"""Remap ingest stage (klt_set_remap): kernel time of its launch beside the level-0 launch of the same build, by the dispatches' own
timestamps (klt_timing_enable 2: remap_kernel is the family remap, the level-0 launch smooth_grad_l0).  At 1080p and at 4K, for one frame
and for a batch of `--batch` frames in one build, under an identity map, a barrel undistortion (KLTUndistortMap, k1 -0.25, k2 0.05) and a
rotation by 10 degrees about the centre.  Every build is of freshly uploaded frames, so every build remaps; medians of `--reps` builds
after `--warmup`.  Besides, on the same frames with the map off and CLAHE on (8 x 8 tiles, clip limit 3.0): clahe_apply_kernel (the
family equalize_apply), the existing kernel with the nearest shape.  Per case the bytes the remap launch moves per frame -- the map (8
bytes a pixel, read once per launch, so divided by the frames of the build) + 1 byte read + 1 byte written per pixel -- and its ratio to
the level-0 launch and to clahe_apply_kernel.  One JSON line, also written to `--out`.
`python tools/remap_probe.py [--reps 15] [--warmup 5] [--batch 16] [--out profiles/remap_probe.json]`."""
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
from pyfeaturetrack_amd.params import KLTUndistortMap                  # noqa: E402


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def maps(width, height):
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    cx, cy, a = (width - 1) / 2.0, (height - 1) / 2.0, np.deg2rad(10.0)
    f = np.hypot(width, height) / 2.0
    barrel = KLTUndistortMap(width, height, [[f, 0, cx], [0, f, cy], [0, 0, 1]], (-0.25, 0.05, 0.0, 0.0))
    to_entries = lambda v: np.rint(256.0 * v).astype(np.int32)           # noqa: E731
    return {"identity": (to_entries(x), to_entries(y)),
            "barrel": (barrel.map_x, barrel.map_y),
            "rotation": (to_entries(cx + np.cos(a) * (x - cx) - np.sin(a) * (y - cy)), to_entries(cy + np.sin(a) * (x - cx) + np.cos(a) * (y - cy)))}


def builds(cx, frames, families, reps, warmup):
    """microseconds per build of each family: `frames` uploaded into slots 0 .. and built in one call, again and again"""
    slots = list(range(len(frames)))
    us = {f: [] for f in families}
    for r in range(warmup + reps):
        for s, f in zip(slots, frames):
            cx.upload(s, f)
        cx.timing_enable(2)
        cx.build_pyramids_batch(slots, sync=True)
        e = {e["name"]: e for e in cx.timing_read()}
        cx.timing_enable(0)
        assert all(e[f]["launches"] == 1 for f in families), e
        if r >= warmup:
            for f in families:
                us[f].append(e[f]["total_ms"] * 1e3)
    return {f: stats(v) for f, v in us.items()}


def shape(cx, res, name, width, height, batch, reps, warmup):
    out = res[name] = {"width": width, "height": height}
    random = [synth.synth_pair(width, height, seed=1 + k)[0] for k in range(2)]
    tables = maps(width, height)
    for count in (1, batch):
        form = out["frames_%d" % count] = {}
        frames = [random[k % 2] for k in range(count)]
        cx.set_remap()
        cx.set_equalize_params(mode=1, tiles_x=8, tiles_y=8, clip_q8=768)
        form["clahe"] = builds(cx, frames, ("equalize_apply", "smooth_grad_l0"), reps, warmup)
        cx.set_equalize_params(mode=0)
        apply_us = form["clahe"]["equalize_apply"]["median"]
        form["bytes_per_frame"] = int(width * height * (8.0 / count + 2.0))
        for kind, (mx, my) in tables.items():
            cx.set_remap(mx, my)
            got = form[kind] = builds(cx, frames, ("remap", "smooth_grad_l0"), reps, warmup)
            assert cx.remap_path() == 1
            got["remap_over_level0"] = round(got["remap"]["median"] / got["smooth_grad_l0"]["median"], 3)
            got["remap_over_clahe_apply"] = round(got["remap"]["median"] / apply_us, 3)
            got["gbytes_per_s"] = round(form["bytes_per_frame"] * count / (got["remap"]["median"] * 1e-6) / 1e9, 1)
    cx.set_remap()
    for s in range(batch):
        cx.slot_free(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_probe.json"))
    a = ap.parse_args()
    tc = KLT_TrackingContext()
    tc.window_width = tc.window_height = 7
    tc.nPyramidLevels, tc.subsampling = 3, 4
    tc.KLTUpdateTCBorder()
    cx = Context(0)
    cx.configure(tc)
    res = {"tool": "tools/remap_probe.py", "reps": a.reps, "warmup": a.warmup, "batch": a.batch,
           "unit": "microseconds per launch, dispatch timestamps; bytes_per_frame: map / frames of the build + 1 read + 1 written per pixel"}
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
