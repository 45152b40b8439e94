"""Shared helpers for the parity tests."""
import hashlib

import numpy as np

from pyfeaturetrack_amd import synth
from pyfeaturetrack_amd.klt import KLT_TrackingContext
from pyfeaturetrack_amd.params import params_from_tc


def sha_bytes(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make_tc(levels=None, ss=None, window=None, **attrs):
    tc = KLT_TrackingContext()
    if window is not None:
        tc.window_width = tc.window_height = window
    if levels is not None:
        tc.nPyramidLevels = levels
        tc.subsampling = ss
    tc.KLTUpdateTCBorder()
    for k, v in attrs.items():
        setattr(tc, k, v)
    return tc


def synth251_frames():
    base = synth.synth_base(251, 187, 11)
    return [synth.synth_frame(251, 187, 11, k, shift=(1.3, -0.8), base=base) for k in range(3)]


def feats_equal(fl, gx, gy, gv):
    """structured feature array vs golden (x, y as float64, val)"""
    return (np.array_equal(fl["val"].astype(np.int64), gv)
            and np.array_equal(fl["x"].astype(np.float64), gx)
            and np.array_equal(fl["y"].astype(np.float64), gy))


__all__ = ["sha_bytes", "make_tc", "synth251_frames", "feats_equal", "params_from_tc"]


# ---- BASELINE-size cases pinned by tests/golden/baseline_sizes.npz (generated from the reference itself, gen_golden.py) ----
def baseline_case(tag):
    """(frames [2 x uint8], tracking context, nFeatures) of the cfg-2 / cfg-3 / cfg-4 / cfg-5 golden cases."""
    if tag == "cfg2":
        return list(synth.synth_pair(1920, 1080, seed=1)), make_tc(levels=3, ss=4), 5000
    if tag == "cfg4":
        return list(synth.synth_pair(1280, 720, seed=0)), make_tc(levels=3, ss=4), 2000
    if tag == "cfg3":
        base = synth.synth_base(1920, 1080, 1)
        return ([synth.synth_frame(1920, 1080, 1, k, shift=(1.1, -0.7), base=base) for k in range(2)],
                make_tc(levels=4, ss=2, window=15), 5000)
    if tag == "cfg5":
        base = synth.synth_base(3840, 2160, 4)
        return ([synth.synth_frame(3840, 2160, 4, k, base=base) for k in range(2)],
                make_tc(levels=3, ss=4, max_residue=10.0), 20000)
    raise KeyError(tag)


def golden_feats_equal(fl, g, tag, what):
    """feature records vs the golden (x, y stored as f32: every value the reference produces is f32-valued)"""
    return (np.array_equal(fl["val"], g["%s_%s_val" % (tag, what)])
            and np.array_equal(fl["x"], g["%s_%s_x" % (tag, what)]) and np.array_equal(fl["y"], g["%s_%s_y" % (tag, what)]))


__all__ += ["baseline_case", "golden_feats_equal"]


# ---- random parameter draws pinned by tests/golden/random_draws.npz (the reference itself ran them: gen_random_draws.py) ----
def random_draws(golden_dir, name="random_draws.npz"):
    """[(draw parameters (+ "frame2", "sequential"), tracking context, frame 0, frame 1, {stage: (x, y, val)})] of the reference's
    random-draw goldens; stages: sel(ected on frame 0), tr(ac)k(ed into frame 1), rep(laced on frame 1), trk2 (tracked into frame 2)."""
    import json
    import os
    g = np.load(os.path.join(golden_dir, name))
    cases = []
    for k, t in enumerate(json.loads(bytes(g["draws_json"]).decode())):
        tc = make_tc(levels=t["levels"], ss=t["ss"], window=t["window"], max_residue=t["mr"], mindist=t["mindist"],
                     nSkippedPixels=t["skip"], smoothBeforeSelecting=t["smooth"], min_eigenvalue=t["min_eig"], max_iterations=t["max_iter"])
        base = synth.synth_base(t["w"], t["h"], t["seed"])
        want = {st: (g["d%d_%s_x" % (k, st)], g["d%d_%s_y" % (k, st)], g["d%d_%s_val" % (k, st)]) for st in ("sel", "trk", "rep", "trk2")}
        t["frame2"] = synth.shift_frame(base, 2 * t["shift"][0], 2 * t["shift"][1])       # the frame of the second tracking call
        t["sequential"] = bool(t["seed"] & 1)                                             # (the reference ran it in sequential mode)
        cases.append((t, tc, synth.shift_frame(base, 0, 0), synth.shift_frame(base, *t["shift"]), want))
    return cases


def draw_equal(fl, want):
    return np.array_equal(fl["val"], want[2]) and np.array_equal(fl["x"], want[0]) and np.array_equal(fl["y"], want[1])


__all__ += ["random_draws", "draw_equal"]


# ---- shared by the GPU tests of the reference-shaped Python API ----
import os as _os                      # noqa: E402

import pytest as _pytest              # noqa: E402


def _api_modules():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf
    from pyfeaturetrack_amd import trackFeatures as trk
    sgf.KLT_verbose = trk.KLT_verbose = 0
    return sgf, trk


def _records(fl):
    return [(f.x, f.y, f.val) for f in fl]


# tests of DEFAULT behaviours that an environment switch changes for the whole process are meaningless under that switch, not wrong
default_cache = _pytest.mark.skipif(bool(_os.environ.get("KLT_NO_FRAME_CACHE") or _os.environ.get("KLT_TRUST_FRAME_IDENTITY")),
                                    reason="the frame cache's default was changed through the environment")
default_lists = _pytest.mark.skipif(bool(_os.environ.get("KLT_NO_FEATURE_RECYCLING") == "1" or _os.environ.get("KLT_LAZY_FEATURE_LISTS") == "1"),
                                    reason="feature lists are lazy / not recycled through the environment")


def colour_of(grey):
    """uint8 [h, w] -> uint8 [h, w, 3]: how the colour test images are made from tests/golden/img0.pgm / img1.pgm -- the same three lines as
    in tests/golden/gen_colour_images.py (three different functions of the frame, so that the luma is not the frame itself)"""
    g = np.asarray(grey, np.uint8)
    return np.dstack([g, np.roll(g, 3, axis=1), (255 - g // 2).astype(np.uint8)])


def assert_dumped_cfg2_pair(dump_dir, row, seed):
    """row `row` of what `bench.py --dump-outputs DIR` wrote (x.npy, y.npy, val.npy) = the CPU oracle's selection + tracking of the cfg-2
    pair of seed `seed`"""
    from benchlib.common import NFEAT, TOL_PX, cfg2_context, oracle_track, records_equal
    from oracle import klt_oracle as ko
    p = params_from_tc(cfg2_context())
    f0, f1 = synth.synth_pair(1920, 1080, seed=seed)
    ko.set_threads(8)
    sel = ko.select_good_features(p, f0.astype(np.float32), NFEAT)
    ko.set_threads(1)
    want = oracle_track(ko, p, f0, f1, sel, threads=8)
    got = np.zeros(NFEAT, want.dtype)
    for k in ("x", "y", "val"):
        got[k] = np.load(_os.path.join(dump_dir, k + ".npy"))[row]
    same, dx = records_equal(got, want)
    assert same and dx <= TOL_PX, (row, seed, dx)
