#!/usr/bin/env python3
"""A parallax scene under both consensus checks.  The camera steps sideways past two depths: the far texture moves 3 px along the rows, the
near one (the lowest third of the frame) 8 px, and a rectangle of a third texture moves 5 px DOWN the columns on its own.  No affine map
describes the two depths at once, so tc.motionModelCheck = "affine" keeps one of them and rejects the other.  tc.epipolarCheck = True finds
the pair's fundamental matrix instead -- here the epipolar lines are the rows -- keeps both depths, and rejects the rectangle, which is off
every epipolar line (KLT_EPIPOLAR_OUTLIER); tc.epipolar_last holds the record, backend.epipolar_matrix turns it into F in pixels.

    python examples/epipolar_check.py [--size 640x480] [--features 400] [--max-error 0.5]
"""
from __future__ import print_function

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.backend import epipolar_matrix                                # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=400)
    ap.add_argument("--max-error", type=float, default=0.5)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0

    far, near, other = (synth.synth_base(w, h, s) for s in (21, 23, 22))
    y0, y1, x0, x1 = h // 6, h // 2, w // 3, 2 * w // 3
    near_from = 2 * h // 3

    def frame(k):
        f = synth.shift_frame(far, 3.0 * k, 0.0)
        f[near_from:] = synth.shift_frame(near, 8.0 * k, 0.0)[near_from:]
        f[y0:y1, x0:x1] = synth.shift_frame(other, 0.0, 5.0 * k)[y0:y1, x0:x1]         # the rectangle: other texture that moves on its own
        return f

    f0, f1 = frame(0), frame(1)

    def run(**switches):
        tc = KLT_TrackingContext()
        tc.nPyramidLevels, tc.subsampling = 3, 2
        tc.KLTUpdateTCBorder()
        for k, v in switches.items():
            setattr(tc, k, v)
        fl = sgf.KLTSelectGoodFeatures(tc, f0, args.features)
        start = [(f.x, f.y) for f in fl]
        tf.KLTTrackFeatures(tc, f0, f1, fl)
        return tc, fl, start

    _, plain, start = run()
    _, affine, _ = run(motionModelCheck="affine", model_max_error=args.max_error)
    tc, epipolar, _ = run(epipolarCheck=True, epipolar_max_error=args.max_error)
    tracked = [f.val == kltState.KLT_TRACKED for f in plain]
    where = []
    for x, y in start:
        if x0 + 8 <= x < x1 - 8 and y0 + 8 <= y < y1 - 8:
            where.append("rectangle")
        elif y >= near_from + 8:
            where.append("near")
        elif y < near_from - 8 and not (x0 - 8 <= x < x1 + 8 and y0 - 8 <= y < y1 + 8):
            where.append("far")
        else:
            where.append("edge")
    print("%-10s %8s %22s %22s" % ("", "tracked", "affine check rejects", "epipolar check rejects"))
    for part in ("far", "near", "rectangle", "edge"):
        sel = [t and p == part for t, p in zip(tracked, where)]
        print("%-10s %8d %22d %22d" % (part, sum(sel), sum(s and f.val == kltState.KLT_MODEL_OUTLIER for s, f in zip(sel, affine)),
                                       sum(s and f.val == kltState.KLT_EPIPOLAR_OUTLIER for s, f in zip(sel, epipolar))))
    m = tc.epipolar_last
    print("epipolar model: valid %d, %d of %d candidates are inliers (hypothesis %d)" % (m["valid"], m["n_inliers"], m["n_candidates"], m["hypothesis"]))
    F = epipolar_matrix(m)
    if F is not None:
        print("  F in pixels (a sideways step is [[0, 0, 0], [0, 0, -1], [0, 1, 0]] / sqrt(2), up to its sign):")
        for row in F:
            print("    [% .5f % .5f % .5f]" % tuple(row))


if __name__ == "__main__":
    main()
