#!/usr/bin/env python3
"""Track identities through an occlusion with KLTTrackSequence.  The clip of examples/reacquire.py -- a textured scene drifts across the
frame, for some frames a flat block covers part of it -- tracked in ONE call, every step enqueued on the device.  Without
tc.reacquireLost a slot's identity ends when its track is lost: the table holds `val > 0` rows and nothing connects the corner that
comes back to the track it was.  With the switch, `ft.ident` carries a persistent id per slot and frame, and a corner selected again
within tc.reacquire_radius pixels of where a lost track was last seen, whose descriptor matches it mutually, gets the old id back
(val 3, with the frames it was away in `gap`).  The scene's motion is known here, so every re-acquired identity can be checked against
the corner it began on.

    python examples/reacquire_sequence.py [--size 320x240] [--features 500] [--frames 30] [--cover 6:18] [--radius 24]
"""
from __future__ import print_function

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pyfeaturetrack_amd import selectGoodFeatures as sgf                              # noqa: E402
from pyfeaturetrack_amd import trackFeatures as tf                                    # noqa: E402
from pyfeaturetrack_amd.klt import KLT_TrackingContext                                # noqa: E402
from pyfeaturetrack_amd.trackSequence import KLTTrackSequence                         # noqa: E402
from reacquire import SHIFT, make_clip                                                # noqa: E402


def run(clip, n_features, reacquire, radius):
    """(identities of frame 0 alive at the end, how many of them went through a re-acquisition, how many of those sit on another corner
    than their own, the largest gap)"""
    tc = KLT_TrackingContext()
    tc.mindist = 12
    tc.max_residue = 10.0
    tc.reacquireLost = reacquire
    tc.reacquire_radius = radius
    ft = KLTTrackSequence(tc, clip, n_features)
    rec, last = ft.rec, len(clip) - 1
    if not reacquire:                        # no ids: an identity of frame 0 lives as long as its slot is tracked without a break
        alive = rec[0]["val"] >= 0
        for k in range(1, len(clip)):
            alive &= rec[k]["val"] == 0
        return int(alive.sum()), 0, 0, -1
    ident = ft.ident
    again = set(int(i) for i in ident["id"][ident["val"] == 3])
    alive = [(s, int(i)) for s, i in enumerate(ident[last]["id"]) if ident[last]["val"][s] != 0 and 0 <= i < n_features]
    regained = [(s, i) for s, i in alive if i in again]
    wrong = 0
    for s, i in regained:                    # identity i began in slot i of frame 0
        if (abs(rec[last]["x"][s] - last * SHIFT[0] - rec[0]["x"][i]) > 2.0 or abs(rec[last]["y"][s] - last * SHIFT[1] - rec[0]["y"][i]) > 2.0):
            wrong += 1
    gaps = ident["gap"][ident["val"] == 3]
    return len(alive), len(regained), wrong, int(gaps.max()) if len(gaps) else -1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x240")
    ap.add_argument("--features", type=int, default=500)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--cover", default="6:18")
    ap.add_argument("--radius", type=int, default=24)
    args = ap.parse_args(argv)
    w, h = (int(v) for v in args.size.split("x"))
    cover = tuple(int(v) for v in args.cover.split(":"))
    sgf.KLT_verbose = tf.KLT_verbose = 0
    clip = make_clip(w, h, args.frames, cover)
    results = {}
    for reacquire in (False, True):
        alive, regained, wrong, gap = results[reacquire] = run(clip, args.features, reacquire, args.radius)
        print("%-24s %4d identities of frame 0 alive after %d frames (%d re-acquired, %d of them on another corner; longest gap %d)"
              % ("tc.reacquireLost = True:" if reacquire else "tc.reacquireLost = False:", alive, args.frames, regained, wrong, gap))
    return results


if __name__ == "__main__":
    main()
