#!/usr/bin/env python3
"""The motion-model check on a pair with an independently moving block: the background moves by (1.3, -0.8), a rectangle of other texture
moves by (-2.5, +3.0).  The features on the rectangle track perfectly well -- the forward-backward check keeps them -- and are wrong for
the scene's motion.  With tc.motionModelCheck = "affine" the frame pair's dominant affine motion is found among the tracks on the device
and every tracked feature further than tc.model_max_error px from it comes back lost (KLT_MODEL_OUTLIER); tc.model_last holds the map.

    python examples/motion_model.py [--size 640x480] [--features 300] [--max-error 1.0]
"""
from __future__ import print_function

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTCountRemainingFeatures, kltState     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--max-error", type=float, default=1.0)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0

    base, other = synth.synth_base(w, h, 21), synth.synth_base(w, h, 22)
    f0, f1 = synth.shift_frame(base, 0.0, 0.0), synth.shift_frame(base, 1.3, -0.8)
    y0, y1, x0, x1 = h // 4, 3 * h // 4, w // 3, 2 * w // 3
    f0[y0:y1, x0:x1] = synth.shift_frame(other, 0.0, 0.0)[y0:y1, x0:x1]                 # the block: other texture ...
    f1[y0:y1, x0:x1] = synth.shift_frame(other, -2.5, 3.0)[y0:y1, x0:x1]                # ... that moves on its own

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
    _, fb, _ = run(forwardBackwardCheck=True, fb_max_error=1.0)
    tc, model, _ = run(motionModelCheck="affine", model_max_error=args.max_error)
    on_block = [x0 + 8 <= x < x1 - 8 and y0 + 8 <= y < y1 - 8 for x, y in start]
    tracked = [f.val == kltState.KLT_TRACKED for f in plain]
    fb_rejected = [t and f.val == kltState.KLT_FB_INCONSISTENT for t, f in zip(tracked, fb)]
    flagged = [f.val == kltState.KLT_MODEL_OUTLIER for f in model]
    print("features selected:                        %d (%d well inside the block)" % (len(start), sum(on_block)))
    print("tracked by the plain tracker:             %d (%d of them on the block)" % (
        KLTCountRemainingFeatures(plain), sum(b and t for b, t in zip(on_block, tracked))))
    print("rejected by the forward-backward check:   %d (%d on the block)" % (sum(fb_rejected), sum(b and r for b, r in zip(on_block, fb_rejected))))
    print("rejected by the motion-model check:       %d (%d on the block)" % (sum(flagged), sum(b and r for b, r in zip(on_block, flagged))))
    m = tc.model_last
    print("model: valid %d, %d of %d candidates are inliers (hypothesis %d)" % (m["valid"], m["inliers"], m["candidates"], m["hypothesis"]))
    if m["A"] is not None:
        print("  A = [[%.5f, %.5f], [%.5f, %.5f]]   t = (%.3f, %.3f)   (the background moved by (1.3, -0.8))"
              % (m["A"][0, 0], m["A"][0, 1], m["A"][1, 0], m["A"][1, 1], m["t"][0], m["t"][1]))


if __name__ == "__main__":
    main()
