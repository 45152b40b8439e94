#!/usr/bin/env python3
"""A camera that backs away, with and without the crowding check.  Every frame is the first one's texture scaled about the frame
centre, so the tracks move towards each other.  Selection placed the features tc.mindist apart and the replacement pass keeps every NEW
feature that far from the live ones -- but nothing keeps the live ones apart once they move: without the check the live features pile
up, with tc.crowdingCheck = True the younger of two tracks that come within tc.mindist of each other is dropped (KLT_CROWDED) and its
slot refilled elsewhere by the same frame's replacement pass.  ft.crowd holds every slot's age, and the track a dropped one merged into.

    python examples/crowding_check.py [--size 640x480] [--features 600] [--frames 16] [--zoom 0.97]
"""
from __future__ import print_function

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState                      # noqa: E402
from pyfeaturetrack_amd.trackSequence import KLTTrackSequence                         # noqa: E402


def close_pairs(row, r):
    """pairs of live features whose pixels are within r of each other in x and in y"""
    live = row["val"] >= 0
    px, py = row["x"][live].astype(np.int64), row["y"][live].astype(np.int64)
    close = (np.abs(px[:, None] - px[None, :]) <= r) & (np.abs(py[:, None] - py[None, :]) <= r)
    return (int(close.sum()) - len(px)) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=600)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--zoom", type=float, default=0.97)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0
    base = synth.synth_base(w, h, 31)
    frames = [synth.warp_frame(base, np.eye(2) * args.zoom ** k) for k in range(args.frames)]

    def run(check):
        tc = KLT_TrackingContext()
        tc.nPyramidLevels, tc.subsampling = 2, 4
        tc.KLTUpdateTCBorder()
        tc.crowdingCheck = check
        return tc, KLTTrackSequence(tc, frames, args.features)

    tc, plain = run(False)
    _, checked = run(True)
    r = tc.mindist - 1
    print("live features closer than mindist = %d (pairs within %d px), frame by frame" % (tc.mindist, r))
    print("%5s %14s %14s %10s %12s" % ("frame", "check off", "check on", "dropped", "oldest track"))
    for k in range(args.frames):
        print("%5d %14d %14d %10d %12d" % (k, close_pairs(plain.rec[k], r), close_pairs(checked.rec[k], r),
                                           int((checked.crowd[k]["val"] == 2).sum()), int(checked.crowd[k]["age"].max())))
    last = checked.crowd[-1]
    merged = np.flatnonzero(last["val"] == 2)
    if merged.size:
        i = int(merged[0])
        print("in the last frame slot %d was dropped: it had come within %d px of slot %d, tracked for %d frames" % (
            i, r, last["winner"][i], last["age"][last["winner"][i]]))
    assert not (plain.rec["val"] == kltState.KLT_CROWDED).any()


if __name__ == "__main__":
    main()
