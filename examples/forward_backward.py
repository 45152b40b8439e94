#!/usr/bin/env python3
"""The forward-backward consistency check on a pair with an occluded block: features selected on frame 0 are tracked into frame 1, where
a rectangle has been replaced by unrelated texture.  Without the check the tracker reports many of the features under the rectangle as
tracked (they slid onto something similar enough); with tc.forwardBackwardCheck each feature is also tracked back into frame 0 and
rejected (KLT_FB_INCONSISTENT) unless it lands within tc.fb_max_error pixels of where it started -- one fused kernel launch.

    python examples/forward_backward.py [--size 640x480] [--features 400] [--max-error 1.0] [--out fb_rejected.ppm]
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
from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTCountRemainingFeatures, kltState     # noqa: E402


def write_ppm(path, gray, marks):
    """the frame in grey with a 5x5 square per mark: (x, y, (r, g, b))"""
    rgb = np.repeat(gray[:, :, None], 3, axis=2)
    h, w = gray.shape
    for x, y, colour in marks:
        xi, yi = int(round(x)), int(round(y))
        rgb[max(0, yi - 2):min(h, yi + 3), max(0, xi - 2):min(w, xi + 3)] = colour
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(rgb.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=400)
    ap.add_argument("--max-error", type=float, default=1.0)
    ap.add_argument("--out", default="fb_rejected.ppm")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0

    base = synth.synth_base(w, h, 21)
    f0, f1 = synth.shift_frame(base, 0.0, 0.0), synth.shift_frame(base, 1.3, -0.8)
    y0, y1, x0, x1 = h // 4, 3 * h // 4, w // 3, 2 * w // 3
    f1[y0:y1, x0:x1] = synth.shift_frame(synth.synth_base(w, h, 22), 0.0, 0.0)[y0:y1, x0:x1]      # the occluder

    def run(check):
        tc = KLT_TrackingContext()
        tc.nPyramidLevels, tc.subsampling = 3, 2
        tc.KLTUpdateTCBorder()
        tc.forwardBackwardCheck, tc.fb_max_error = check, args.max_error
        fl = sgf.KLTSelectGoodFeatures(tc, f0, args.features)
        start = [(f.x, f.y) for f in fl]
        tf.KLTTrackFeatures(tc, f0, f1, fl)
        return fl, start

    plain, start = run(False)
    checked, _ = run(True)
    under = [x0 <= x < x1 and y0 <= y < y1 for x, y in start]
    rejected = [f.val == kltState.KLT_FB_INCONSISTENT for f in checked]
    print("features selected:                 %d (%d under the occluded block)" % (len(start), sum(under)))
    print("tracked without the check:         %d (%d of them started under the block)" % (
        KLTCountRemainingFeatures(plain), sum(u and f.val >= 0 for u, f in zip(under, plain))))
    print("tracked with the check:            %d (%d of them started under the block)" % (
        KLTCountRemainingFeatures(checked), sum(u and f.val >= 0 for u, f in zip(under, checked))))
    print("rejected as inconsistent:          %d (%d under the block)" % (sum(rejected), sum(u and r for u, r in zip(under, rejected))))
    marks = [(f.x, f.y, (0, 255, 0)) for f in checked if f.val >= 0]
    marks += [(p.x, p.y, (255, 0, 0)) for p, r in zip(plain, rejected) if r]       # where the plain tracker had put the rejected ones
    write_ppm(args.out, f1, marks)
    print("wrote %s: kept features green, rejected ones red (at the position the plain tracker reported)" % args.out)


if __name__ == "__main__":
    main()
