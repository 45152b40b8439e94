#!/usr/bin/env python3
"""A panning camera under all three consensus checks.  The camera pans with perspective: the whole background moves by ONE homography
(a few pixels, its perspective part about a pixel across the frame), and a rectangle of another texture moves 5 px DOWN the columns on its
own.  An affine map cannot follow the perspective part, so tc.motionModelCheck = "affine" rejects good tracks towards the frame's corners
(a third of the background); under a homography the fundamental matrix is not unique, so tc.epipolarCheck = True finds one that fits the
rectangle too and lets it through; tc.homographyCheck = True finds the homography, keeps the background and rejects the rectangle
(KLT_HOMOGRAPHY_OUTLIER).
tc.homography_last holds the record, backend.homography_matrix turns it into H in pixels.

    python examples/homography_check.py [--size 640x480] [--features 400] [--max-error 0.5]
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
from pyfeaturetrack_amd.backend import homography_matrix                              # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=400)
    ap.add_argument("--max-error", type=float, default=0.5)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0

    back, other = synth.synth_base(w, h, 21), synth.synth_base(w, h, 22)
    y0, y1, x0, x1 = h // 6, h // 2, w // 3, 2 * w // 3
    # the pan: about the frame centre, 3 px and 1.5 px of shift, a slight roll, and a perspective part of 1.5 px at the corners
    c = np.array([[1, 0, w / 2.0], [0, 1, h / 2.0], [0, 0, 1.0]])
    g = 1.5 / ((w / 2.0) ** 2)
    H_true = c @ np.array([[1.0, 0.004, 3.0], [-0.004, 1.0, 1.5], [g, 0.5 * g, 1.0]]) @ np.linalg.inv(c)

    def frame(k):
        f = synth.warp_homography(back, np.linalg.matrix_power(H_true, k))
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
    _, epipolar, _ = run(epipolarCheck=True, epipolar_max_error=args.max_error)
    tc, homography, _ = run(homographyCheck=True, homography_max_error=args.max_error)
    tracked = [f.val == kltState.KLT_TRACKED for f in plain]
    where = []
    for x, y in start:
        if x0 + 8 <= x < x1 - 8 and y0 + 8 <= y < y1 - 8:
            where.append("rectangle")
        elif not (x0 - 8 <= x < x1 + 8 and y0 - 8 <= y < y1 + 8):
            where.append("background")
        else:
            where.append("edge")
    print("%-10s %8s %22s %24s %26s" % ("", "tracked", "affine check rejects", "epipolar check rejects", "homography check rejects"))
    for part in ("background", "rectangle", "edge"):
        sel = [t and p == part for t, p in zip(tracked, where)]
        print("%-10s %8d %22d %24d %26d" % (part, sum(sel), sum(s and f.val == kltState.KLT_MODEL_OUTLIER for s, f in zip(sel, affine)),
                                            sum(s and f.val == kltState.KLT_EPIPOLAR_OUTLIER for s, f in zip(sel, epipolar)),
                                            sum(s and f.val == kltState.KLT_HOMOGRAPHY_OUTLIER for s, f in zip(sel, homography))))
    m = tc.homography_last
    print("homography model: valid %d, %d of %d candidates are inliers (hypothesis %d)" % (m["valid"], m["n_inliers"], m["n_candidates"], m["hypothesis"]))
    H = homography_matrix(m)
    if H is not None:
        print("  H in pixels, scaled to H[2][2] = 1 (on the right: the camera's)")
        for row, want in zip(H / H[2, 2], H_true / H_true[2, 2]):
            print("    [% .6f % .6f % .4f]      [% .6f % .6f % .4f]" % (tuple(row) + tuple(want)))


if __name__ == "__main__":
    main()
