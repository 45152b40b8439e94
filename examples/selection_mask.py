#!/usr/bin/env python3
"""A selection mask: features are selected on a frame in which a rectangle (a vehicle's bonnet, a burnt-in timestamp, an object a
segmentation model found) must stay free of features.  tc.selectionMask is a [nrows][ncols] array in which 0 marks the pixels that are
never candidates; KLTSelectGoodFeatures, KLTReplaceLostFeatures and KLTTrackSequence honour it, the tracker ignores it.  The selection is
exactly what it would be had the masked pixels never been on the candidate list: the features the rectangle would have taken go to the
next best places outside it.

    python examples/selection_mask.py [--size 640x480] [--features 300] [--out selection_mask.ppm]
"""
from __future__ import print_function

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                                    # noqa: E402

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, KLTCountRemainingFeatures     # noqa: E402


def write_ppm(path, gray, masked, marks):
    """the frame in grey, the masked pixels tinted red, a 5x5 square per mark: (x, y, (r, g, b))"""
    rgb = np.repeat(gray[:, :, None], 3, axis=2)
    rgb[masked, 1:] //= 2
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
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--out", default="selection_mask.ppm")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    sgf.KLT_verbose = 0

    img = synth.shift_frame(synth.synth_base(w, h, 21), 0.0, 0.0)
    y0, y1, x0, x1 = h // 2, h - h // 8, w // 4, w - w // 4
    mask = np.ones((h, w), bool)
    mask[y0:y1, x0:x1] = False                                   # no feature here

    tc = KLT_TrackingContext()
    plain = sgf.KLTSelectGoodFeatures(tc, img, args.features)
    tc.selectionMask = mask
    masked = sgf.KLTSelectGoodFeatures(tc, img, args.features)
    tc.selectionMask = None                                      # (back to selecting anywhere)

    def inside(fl):
        return sum(f.val >= 0 and x0 <= f.x < x1 and y0 <= f.y < y1 for f in fl)
    print("without a mask: %d features, %d inside the rectangle" % (KLTCountRemainingFeatures(plain), inside(plain)))
    print("with the mask:  %d features, %d inside the rectangle" % (KLTCountRemainingFeatures(masked), inside(masked)))
    marks = [(f.x, f.y, (0, 255, 0)) for f in masked if f.val >= 0]
    write_ppm(args.out, img, ~mask, marks)
    print("wrote %s: masked pixels tinted red, selected features green" % args.out)


if __name__ == "__main__":
    main()
