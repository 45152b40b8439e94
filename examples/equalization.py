#!/usr/bin/env python3
"""A frame pair whose left half is dark (v * 0.08 + 5: a backlit scene, a shadow, a thermal camera squeezed into 8 bits): the 7x7 sums
of the selection sit in a few grey levels there, and min_eigenvalue turns away corners a person would pick.  tc.equalization = "clahe"
equalises every frame on the device in front of the pyramid build (contrast-limited adaptive histogram equalisation, DESIGN.md section
9l) and selection finds the dark half again.  Prints the features selected and tracked in each half, with and without the switch.

    python examples/equalization.py [--features 300] [--tiles 8x8] [--clip-limit 3.0]
"""
from __future__ import print_function

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                                    # noqa: E402

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState                      # noqa: E402


def read_pgm(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"), np.uint8)


def darken_left_half(img):
    out = np.array(img, np.uint8)
    half = out.shape[1] // 2
    out[:, :half] = (out[:, :half] * 0.08 + 5).astype(np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--tiles", default="8x8")
    ap.add_argument("--clip-limit", type=float, default=3.0)
    args = ap.parse_args()
    tiles = tuple(int(v) for v in args.tiles.split("x"))
    sgf.KLT_verbose = tf.KLT_verbose = 0
    golden = os.path.join(ROOT, "tests", "golden")
    frames = [darken_left_half(read_pgm(os.path.join(golden, name))) for name in ("img0.pgm", "img1.pgm")]
    half = frames[0].shape[1] // 2

    print("left half of both frames darkened to v * 0.08 + 5; %d features asked for" % args.features)
    for switch in (None, "clahe"):
        tc = KLT_TrackingContext()
        tc.equalization, tc.clahe_tiles, tc.clahe_clip_limit = switch, tiles, args.clip_limit
        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], args.features)
        x = np.array([f.x for f in fl])
        chosen = np.array([f.val for f in fl]) >= 0
        left = x < half
        tf.KLTTrackFeatures(tc, frames[0], frames[1], fl)
        tracked = chosen & (np.array([f.val for f in fl]) == kltState.KLT_TRACKED)
        print("equalization = %-8r selected %3d (left half %3d, right half %3d), tracked %3d (left half %3d, right half %3d)"
              % (switch, chosen.sum(), (chosen & left).sum(), (chosen & ~left).sum(), tracked.sum(), (tracked & left).sum(), (tracked & ~left).sum()))
    seen = sgf.KLTEqualizeImage(tc, frames[0])
    print("the equalised frame 0 (KLTEqualizeImage): left half grey levels %d .. %d (as sent: %d .. %d)"
          % (seen[:, :half].min(), seen[:, :half].max(), frames[0][:, :half].min(), frames[0][:, :half].max()))


if __name__ == "__main__":
    main()
