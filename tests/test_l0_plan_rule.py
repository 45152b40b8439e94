"""The level-0 launch rule without a GPU: plan_level0 (pyfeaturetrack_amd/csrc/l0_plan.h, plain C++) is compiled with g++ into a small dump
program (tests/l0_plan_dump.cpp) and asked about a sweep of launches; its answers are held against the Python restatements the GPU tests
plan their cases with -- pyramid_expected.expected_path, test_gpu_l0_wide.takes_wide / wide_grid, test_gpu_l0_lean_wave.goes_lean /
takes_wave, test_gpu_l0_lean.takes_geometry -- each left as it is.  Drift between the host's rule and any of them fails here, not only
where klt_level0_path disagrees on a GPU.

The restatements speak about builds at subsampling 4 with more than one level and 5 or 9 smoothing taps; the sweep also holds launches
outside that (subsampling 2, one level, 7 smoothing taps), where the answer is expected_path's alone and nothing streams or goes lean.

raw_quads_aligned, the rule in the same header for the quad loads of a caller's frame (an adopted frame starts at any byte), is swept through
the same program against a one-line numpy restatement."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import test_gpu_l0_lean as lean_mod
import test_gpu_l0_lean_wave as wave_mod
import test_gpu_l0_wide as wide_mod
from helpers import make_tc, params_from_tc
from pyramid_expected import MAX_BATCH, RB16, RB32, RB32_HRED, STREAM, STREAM_NO_CENTRE, TALL_PIXELS, TILED_LDS, expected_path

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_WIDE, STREAM_WIDE_NO_CENTRE = wide_mod.STREAM_WIDE, wide_mod.STREAM_WIDE_NO_CENTRE
FAMILY_TILED_LDS, FAMILY_RB_TILE, FAMILY_BANDED, FAMILY_WAVE = range(4)
SIZES = [63, 64, 65, 127, 128, 255, 256, 257, 1024, 1920, 4096]
BATCHES = [1, 2, 9, 10, 16, 31, 32]
SIGMAS = [0.1, 0.15, 0.2]
WAVE_STRIP, WAVE_SEG, WAVE_WAVES = wave_mod.STRIP, wave_mod.SEG, 4
TALL_EDGE = [(1000, 1000, 1), (999, 1000, 1), (1000, 999, 1), (500, 1000, 2)]       # (ncols, nrows, batch): exactly TALL_PIXELS, and just below


def cdiv(a, b):
    return -(-a // b)


def library_taps(k):
    """make_taps (api_frames.hip): the taps reversed, and correlate1d's symmetry class"""
    k = [float(v) for v in k][::-1]
    h, eps = len(k) // 2, 2.220446049250313e-16
    sym = 0
    if len(k) & 1:
        if all(abs(k[h + i] - k[h - i]) <= eps for i in range(1, h + 1)):
            sym = 1
        elif all(abs(k[h + i] + k[h - i]) <= eps for i in range(1, h + 1)):
            sym = -1
    return sym, k


def tap_line(name, sym, k):
    return "T %s %d %d %s" % (name, len(k), sym, " ".join(v.hex() for v in k))


@functools.lru_cache(maxsize=None)
def product_taps(ss, sigma):
    """the four tap sets of a configuration as the library holds them: smoothing, gradient Gaussian, gradient derivative, reduction"""
    from pyfeaturetrack_amd.params import taps_from_params
    (sg, _), (rg, _), (gg, gd) = taps_from_params(params_from_tc(make_tc(levels=2, ss=ss, smooth_sigma_fact=sigma)))
    return [library_taps(t) for t in (sg, gg, gd, rg)]


class Sweep:
    """the requests, one line each, and what every one was asked with"""

    def __init__(self):
        self.lines, self.asked, self.names = [], [], {}

    def taps(self, ss, sigma, sets=None):
        key = (ss, sigma) if sets is None else id(sets)
        if key not in self.names:
            sets = sets or product_taps(ss, sigma)
            self.names[key] = ["t%d_%d" % (len(self.names), i) for i in range(4)]
            self.lines += [tap_line(n, sym, k) for n, (sym, k) in zip(self.names[key], sets)]
        return self.names[key]

    def add(self, ncols, nrows, batch, f32, sigma=0.1, ss=4, stream=2, form=1, want_hred=1, want_lean=0, kind=None, uniform=1, fuse=1,
            tuning=(0, 0, 0), sets=None, **note):
        kind = (1 if f32 else 0) if kind is None else kind
        names = self.taps(ss, sigma, sets)
        self.lines.append("R %d %d %d %d %d %s %d %d %d %d %d %d %d %d %d" % (
            (ncols, nrows, batch, kind, uniform, " ".join(names), ss, fuse, stream, form, want_hred, want_lean) + tuple(tuning)))
        self.asked.append(dict(ncols=ncols, nrows=nrows, batch=batch, f32=f32, sigma=sigma, ss=ss, stream=stream, form=form,
                               want_hred=want_hred, want_lean=want_lean, kind=kind, uniform=uniform, tuning=tuning, **note))


def edge_shapes():
    """the smallest shapes the GPU tests' own shape functions produce, and the same with one row or one column less: (ncols, nrows)"""
    out = [(nc, nr) for nc, nr, _ in wide_mod.SHAPES]
    out += [(nc, nr) for _, nc, nr, _ in lean_mod.CASES]
    out += [(nc, nr) for _, nc, nr, _ in wave_mod.shapes()]
    return sorted(set(out) | {(nc - 1, nr) for nc, nr in out} | {(nc, nr - 1) for nc, nr in out})


def wishes(ss):
    """(stream, want_hred, want_lean, form): every option value with both wishes on and off; the lean form option where lean is asked for"""
    if ss != 4:
        return [(1, h, 0, 1) for h in (0, 1)]
    return [(s, h, l, f) for s in (0, 1, 2) for h in (0, 1) for l, f in ((0, 1), (1, 0), (1, 1))]


def build_sweep():
    sw = Sweep()
    for ss, sigma in itertools.product((4, 2), SIGMAS):
        shapes = list(itertools.product(SIZES, SIZES + [1080], BATCHES)) + [(nc, nr, MAX_BATCH) for nc, nr in edge_shapes()] + TALL_EDGE
        for (nc, nr, batch), f32, (stream, hred, lean, form) in itertools.product(shapes, (False, True), wishes(ss)):
            sw.add(nc, nr, batch, f32, sigma, ss, stream, form, hred, lean, what="sweep")
    # gradient launches (kinds 2 and 3): the tile by the same pixel count, per-entry geometry, no wish honoured
    for (nc, nr, batch), kind, uniform in itertools.product([(480, 270, 16), (480, 270, 2), (256, 128, 31), (1920, 1080, 1)], (2, 3), (0, 1)):
        sw.add(nc, nr, batch, kind == 2, kind=kind, uniform=uniform, want_lean=1, what="gradients")
    # the centre-tap elision: u8 frames whose derivative centre is -0.0, a smoothing tap with a sign bit (-0.0 at the far end: still symmetric)
    base = product_taps(4, 0.1)
    minus_centre = [base[0], base[1], (base[2][0], [(-0.0 if i == len(base[2][1]) // 2 else v) for i, v in enumerate(base[2][1])]), base[3]]
    signed_smooth = [(1, [-0.0] + base[0][1][1:-1] + [-0.0])] + base[1:]
    for sets, what in ((None, "elidable"), (minus_centre, "centre -0.0"), (signed_smooth, "signed smoothing tap")):
        for f32, lean in itertools.product((False, True), (0, 1)):
            sw.add(1920, 1080, 16, f32, want_lean=lean, sets=sets, what=what)
    # a frame whose entries differ in size has no wave form
    sw.add(1920, 1080, 16, False, want_lean=1, uniform=0, what="non-uniform lean")
    # the three experiment hooks: tile height, segment height (banded: only where the band divides it; the wave form: any), wide grid bound
    sw.add(256, 128, 2, False, want_hred=0, tuning=(32, 0, 0), what="KLT_RB_TH")
    sw.add(1920, 1080, 16, False, stream=1, tuning=(0, 48, 0), what="KLT_L0_SEG narrow 48")          # 32 does not divide 48: stays 160
    sw.add(1920, 1080, 16, False, tuning=(0, 48, 0), what="KLT_L0_SEG wide 48")                        # 16 does
    sw.add(1920, 1080, 16, False, want_lean=1, tuning=(0, 50, 0), what="KLT_L0_SEG wave 50")
    sw.add(1920, 1080, 9, False, tuning=(0, 0, 1000), what="KLT_L0_WIDE_WGS")                          # 15 x 9 x 9 = 1215 workgroups
    return sw


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("l0_plan") / "l0_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
                    "-I" + os.path.join(REPO, "pyfeaturetrack_amd", "csrc"), os.path.join(REPO, "tests", "l0_plan_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def answers(dump_exe):
    exe = dump_exe
    sw = build_sweep()
    r = subprocess.run([exe], input="\n".join(sw.lines) + "\n", capture_output=True, text=True, check=True)
    plans = [{k: int(v) for k, v in (f.split("=") for f in line.split())} for line in r.stdout.splitlines()]
    assert len(plans) == len(sw.asked)
    return list(zip(sw.asked, plans))


def restated(q):
    """what the restatements say about a request of the sweep: (path, lean, lean_form)"""
    sets = product_taps(q["ss"], q["sigma"])
    ns, nreduce = len(sets[0][1]), len(sets[3][1])
    levels = 3 if q["want_hred"] else 1
    narrow = expected_path(q["ncols"], q["nrows"], q["batch"], q["f32"], levels, q["ss"], q["sigma"], stream_opt=min(q["stream"], 1))[0]
    assert narrow == expected_path(q["ncols"], q["nrows"], q["batch"], q["f32"], max(levels - 1, 1), q["ss"], q["sigma"], stream_opt=min(q["stream"], 1))[0]
    # the conditions the size-only restatements take for granted: a caller with levels >= 1, subsampling 4 / 21 taps, 5 or 9 smoothing taps
    fusable = bool(q["want_hred"]) and q["ss"] == 4 and nreduce == 21 and ns in (5, 9)
    dims = (q["ncols"], q["nrows"], q["batch"])
    wide = q["stream"] == 2 and fusable and wide_mod.takes_wide(*dims)
    path = (STREAM_WIDE if q["f32"] else STREAM_WIDE_NO_CENTRE) if wide else narrow
    streams = {0: False, 1: lean_mod.takes_geometry("narrow", *dims), 2: wave_mod.goes_lean(*dims)}[q["stream"]]
    lean = bool(q["want_lean"]) and fusable and streams
    form = 0 if not lean else 2 if q["form"] == 1 and wave_mod.takes_wave(q["ncols"], q["nrows"], ns) else 1
    return path, lean, form


def test_the_plan_is_what_the_restatements_say(answers):
    seen_paths, seen_forms = set(), set()
    for q, p in answers:
        if q["what"] != "sweep":
            continue
        path, lean, form = restated(q)
        assert (p["path"], bool(p["lean"]), p["lean_form"]) == (path, lean, form), (q, p)
        assert not q["want_lean"] or p["lean"] == (path in (STREAM, STREAM_NO_CENTRE, STREAM_WIDE, STREAM_WIDE_NO_CENTRE)), (q, p)
        assert p["hred"] == (path >= RB32_HRED) and p["kind"] == q["kind"] and p["zc"] == (not lean and path in (STREAM_NO_CENTRE, STREAM_WIDE_NO_CENTRE)), (q, p)
        seen_paths.add(path)
        seen_forms.add(form)
        # the grid, as the test modules spell it out
        nc, nr, batch = q["ncols"], q["nrows"], q["batch"]
        grid = (p["gx"], p["gy"], p["gz"])
        if form == 2:
            units = cdiv(nc, WAVE_STRIP) * cdiv(nr, WAVE_SEG) * batch
            assert (p["family"], p["units"], grid, p["block"]) == (FAMILY_WAVE, units, (cdiv(units, WAVE_WAVES), 1, 1), 64 * WAVE_WAVES), (q, p)
            assert (p["strip"], p["seg"], p["nstrips"], p["nsegs"]) == (WAVE_STRIP, WAVE_SEG, cdiv(nc, WAVE_STRIP), cdiv(nr, WAVE_SEG)), (q, p)
        elif path in (STREAM_WIDE, STREAM_WIDE_NO_CENTRE, STREAM, STREAM_NO_CENTRE):
            _, strip, seg, _ = lean_mod.GEOMETRIES["wide" if path >= STREAM_WIDE else "narrow"]
            band = wide_mod.WIDE_BAND if path >= STREAM_WIDE else 32
            assert (p["family"], p["strip"], p["band"], p["seg"]) == (FAMILY_BANDED, strip, band, seg), (q, p)
            assert grid == (cdiv(nc, strip), cdiv(nr, seg), batch) and p["block"] == 256 and p["lds"] == 0, (q, p)
            if path >= STREAM_WIDE:
                assert p["gx"] * p["gy"] * p["gz"] == wide_mod.wide_grid(nc, nr, batch)
        elif path == TILED_LDS:
            assert (p["family"], grid, p["block"]) == (FAMILY_TILED_LDS, (cdiv(nc, 64), cdiv(nr, 16), batch), 256) and p["lds"] > 0, (q, p)
        else:
            rows = 16 if path == RB16 else 32
            assert (p["family"], p["tile_rows"], grid, p["block"], p["lds"]) == (FAMILY_RB_TILE, rows, (cdiv(nc, 64), cdiv(nr, rows), batch), 256, 0), (q, p)
    # every fused code and every lean form is reached: a rule change cannot silently empty a branch
    assert seen_paths == {TILED_LDS, RB16, RB32, RB32_HRED, STREAM, STREAM_NO_CENTRE, STREAM_WIDE, STREAM_WIDE_NO_CENTRE}
    assert seen_forms == {0, 1, 2}


def test_gradient_launches_take_the_tile_by_the_pixel_count(answers):
    got = [(q, p) for q, p in answers if q["what"] == "gradients"]
    assert len(got) == 16
    for q, p in got:
        tall = q["ncols"] * q["nrows"] * q["batch"] >= TALL_PIXELS
        assert (p["path"], p["tile_rows"], p["family"]) == ((RB32, 32, FAMILY_RB_TILE) if tall else (RB16, 16, FAMILY_RB_TILE)), (q, p)
        assert (p["hred"], p["lean"], p["lean_form"], p["zc"], p["kind"]) == (0, 0, 0, 0, q["kind"]), (q, p)
        assert (p["gx"], p["gy"], p["gz"]) == (cdiv(q["ncols"], 64), cdiv(q["nrows"], p["tile_rows"]), q["batch"]), (q, p)


def test_centre_tap_elision_and_the_code_a_lean_launch_reports(answers):
    """zc only for a full launch on u8 frames whose taps allow it; a lean launch reports the code the full launch would get and runs the one
    lean instantiation (zc = 0)"""
    got = {(q["what"], q["f32"], q["want_lean"]): p for q, p in answers if q["what"] in ("elidable", "centre -0.0", "signed smoothing tap")}
    assert len(got) == 12
    for (what, f32, lean), p in got.items():
        elidable = what == "elidable" and not f32
        assert p["path"] == (STREAM_WIDE_NO_CENTRE if elidable else STREAM_WIDE), (what, f32, lean, p)
        assert p["zc"] == (elidable and not lean) and p["lean"] == lean and p["lean_form"] == (2 if lean else 0), (what, f32, lean, p)
    (p,) = [p for q, p in answers if q["what"] == "non-uniform lean"]
    assert (p["lean"], p["lean_form"], p["family"], p["strip"]) == (1, 1, FAMILY_BANDED, 128)


def test_the_experiment_hooks(answers):
    got = {q["what"]: p for q, p in answers if q["what"].startswith("KLT_")}
    assert len(got) == 5
    assert (got["KLT_RB_TH"]["path"], got["KLT_RB_TH"]["tile_rows"], got["KLT_RB_TH"]["gy"]) == (RB32, 32, 4)
    assert (got["KLT_L0_SEG narrow 48"]["path"], got["KLT_L0_SEG narrow 48"]["seg"], got["KLT_L0_SEG narrow 48"]["gy"]) == (STREAM_NO_CENTRE, 160, 7)
    assert (got["KLT_L0_SEG wide 48"]["path"], got["KLT_L0_SEG wide 48"]["seg"], got["KLT_L0_SEG wide 48"]["gy"]) == (STREAM_WIDE_NO_CENTRE, 48, 23)
    p = got["KLT_L0_SEG wave 50"]
    assert (p["lean_form"], p["seg"], p["nsegs"], p["units"], p["gx"]) == (2, 50, 22, 9 * 22 * 16, 9 * 22 * 4)
    assert (got["KLT_L0_WIDE_WGS"]["path"], got["KLT_L0_WIDE_WGS"]["gz"]) == (STREAM_WIDE_NO_CENTRE, 9)


def test_quad_loads_go_by_the_address_and_the_width(dump_exe):
    """raw_quads_aligned over every residue of 16 of the address (on several bases, one past 2^32), every ncols % 4 (on several widths) and
    both element sizes: true exactly where the width is a multiple of 4 and the address one of 4 elements"""
    asked = [(base + r, nc + c, eb) for base in (0, 1 << 20, (1 << 33) + 4096, (1 << 47) - 16) for r in range(16)
             for nc in (4, 64, 1920) for c in range(4) for eb in (1, 4)]
    r = subprocess.run([dump_exe], input="".join("Q %d %d %d\n" % q for q in asked), capture_output=True, text=True, check=True)
    got = np.array([int(line.split("=")[1]) for line in r.stdout.splitlines()], bool)
    addr, ncols, eb = (np.array(v, np.uint64) for v in zip(*asked))
    want = (ncols % 4 == 0) & (addr % (4 * eb) == 0)
    assert got.shape == want.shape and np.array_equal(got, want)
    # both answers for either element size, and the u8 and f32 answers differ where the address is a multiple of 4 and not of 16
    assert {(int(e), bool(g)) for e, g in zip(eb, got)} == {(1, False), (1, True), (4, False), (4, True)}
    assert any(g and e == 1 and a % 16 for a, e, g in zip(addr, eb, got))
