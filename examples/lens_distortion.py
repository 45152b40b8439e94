#!/usr/bin/env python3
"""A static scene under a camera pan, seen through a barrel lens (forward Brown-Conrady, k1 < 0).  Between two pinhole views a pan is a
homography, so tc.homographyCheck flags nothing in a static scene; through the lens it is none, and the check flags good tracks toward
the frame's edges.  tc.remap = KLTUndistortMap(...) rectifies every frame on the device in front of the pyramid build (DESIGN.md
section 9m): selection, tracking and the check then work in the rectified frame.  Prints the static tracks the check flags on the raw
frames and on the rectified ones.

    python examples/lens_distortion.py [--features 300] [--k1 -0.22] [--pan 0.02]
"""
from __future__ import print_function

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                                    # noqa: E402

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import synth                                                  # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext, kltState                      # noqa: E402

W, H, FOCAL = 640, 480, 420.0
KLT_HOMOGRAPHY_OUTLIER = -9


def bilinear(img, x, y):
    """img at float positions, edges replicated"""
    x, y = np.clip(x, 0, img.shape[1] - 1.0), np.clip(y, 0, img.shape[0] - 1.0)
    x0, y0 = np.minimum(x.astype(int), img.shape[1] - 2), np.minimum(y.astype(int), img.shape[0] - 2)
    ax, ay = x - x0, y - y0
    f = img.astype(np.float64)
    return (1 - ax) * (1 - ay) * f[y0, x0] + ax * (1 - ay) * f[y0, x0 + 1] + (1 - ax) * ay * f[y0 + 1, x0] + ax * ay * f[y0 + 1, x0 + 1]


def undistorted(xd, yd, k1):
    """normalised distorted coordinates -> normalised pinhole coordinates (fixed-point iteration; only the synthesis needs this way)"""
    x, y = xd.copy(), yd.copy()
    for _ in range(30):
        radial = 1.0 + k1 * (x * x + y * y)
        x, y = xd / radial, yd / radial
    return x, y


def raw_frame(world, pan, k1):
    """what the lens camera sees after a pan of `pan` rad about the vertical axis: each raw pixel -> its pinhole ray -> the ray before the
    pan -> the world texture (a plane at infinity: twice the frame, centred)"""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = undistorted((u - (W - 1) / 2.0) / FOCAL, (v - (H - 1) / 2.0) / FOCAL, k1)
    c, s = np.cos(pan), np.sin(pan)
    X, Z = c * x + s, -s * x + c                      # the ray (x, y, 1) turned about y
    wx, wy = X / Z * FOCAL + (world.shape[1] - 1) / 2.0, y / Z * FOCAL + (world.shape[0] - 1) / 2.0
    return np.clip(np.rint(bilinear(world, wx, wy)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=300)
    ap.add_argument("--k1", type=float, default=-0.22)
    ap.add_argument("--pan", type=float, default=0.02)
    args = ap.parse_args()
    sgf.KLT_verbose = tf.KLT_verbose = 0
    world = synth.synth_base(2 * W, 2 * H, 7)
    frames = [raw_frame(world, k * args.pan, args.k1) for k in range(2)]
    camera = [[FOCAL, 0, (W - 1) / 2.0], [0, FOCAL, (H - 1) / 2.0], [0, 0, 1]]
    table = sgf.KLTUndistortMap(W, H, camera, (args.k1, 0.0, 0.0, 0.0))
    mask = sgf.KLTRemapValidMask(table, margin=2)

    print("a static scene, a pan of %g rad, a barrel lens with k1 = %g; %d features asked for; every flag is a false alarm" % (args.pan, args.k1, args.features))
    for name, remap in (("raw frames", None), ("rectified frames (tc.remap)", table)):
        tc = KLT_TrackingContext()
        tc.homographyCheck = True
        tc.remap = remap
        tc.selectionMask = mask if remap is not None else None       # keep the selection off replicated edges
        fl = sgf.KLTSelectGoodFeatures(tc, frames[0], args.features)
        tf.KLTTrackFeatures(tc, frames[0], frames[1], fl)
        val = np.array([f.val for f in fl])
        print("%-28s tracked %3d, flagged by the homography check %3d" % (name, (val == kltState.KLT_TRACKED).sum(), (val == KLT_HOMOGRAPHY_OUTLIER).sum()))
    seen = sgf.KLTRemapImage(tc, frames[0])
    sx, sy = sgf.KLTRemapSourcePositions(table, np.array([0.0, W - 1.0]), np.array([0.0, H - 1.0]))
    print("the rectified frame 0 (KLTRemapImage) is %d x %d; its corners read the raw frame at (%.1f, %.1f) and (%.1f, %.1f); the mask allows %d of %d pixels"
          % (seen.shape[1], seen.shape[0], sx[0], sy[0], sx[1], sy[1], int(mask.sum()), mask.size))


if __name__ == "__main__":
    main()
