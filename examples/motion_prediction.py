#!/usr/bin/env python3
"""A motion prior on an accelerating pan: the camera's per-frame shift grows by a fixed step, so after a few frames the shift itself is
far outside the tracker's search range while the CHANGE of the shift stays inside it.  KLTTrackSequence is run twice on the clip, without
a prior and with tc.motionPrediction = "constant_velocity" (each feature's search in the next frame starts at its position plus its last
displacement; the prediction and the tracker both run on the device).  Every feature moves with the pan, so a feature is RIGHT when it is
within half a pixel of where the pan has taken it.

    python examples/motion_prediction.py [--size 640x480] [--features 300] [--frames 8] [--step 5.3,1.7]
"""
from __future__ import print_function

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                                    # noqa: E402

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                                # noqa: E402
from pyfeaturetrack_amd.trackSequence import KLTTrackSequence                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--step", default="5.3,1.7", help="growth of the per-frame shift, pixels per frame squared")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    ax, ay = (float(v) for v in args.step.split(","))
    sgf.KLT_verbose = tf.KLT_verbose = 0

    base = synth.synth_base(w, h, 21)
    offsets = [(ax * k * (k + 1) / 2, ay * k * (k + 1) / 2) for k in range(args.frames)]
    frames = [synth.shift_frame(base, ox, oy) for ox, oy in offsets]

    def run(mode):
        tc = KLT_TrackingContext()
        tc.sequentialMode = True
        tc.motionPrediction = mode
        return KLTTrackSequence(tc, iter(frames), args.features, replace_lost=False)

    tables = {"no prior": run(None), "constant velocity": run("constant_velocity")}
    print("frame  shift from the frame before   " + "   ".join("%-28s" % name for name in tables))
    for k in range(1, args.frames):
        cells = []
        for ft in tables.values():
            live = ft.val[k] >= 0
            ex = ft.x[k] - (ft.x[0] + offsets[k][0])
            ey = ft.y[k] - (ft.y[0] + offsets[k][1])
            right = live & (np.hypot(ex, ey) < 0.5)
            cells.append("%4d tracked, %4d right     " % (live.sum(), right.sum()))
        print("%5d  (%6.1f, %6.1f) px            %s" % (k, offsets[k][0] - offsets[k - 1][0], offsets[k][1] - offsets[k - 1][1],
                                                      "   ".join(cells)))


if __name__ == "__main__":
    main()
