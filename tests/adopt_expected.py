"""Adopted frames (klt_slot_adopt_u8) at any address, for the level-0 kernels that read them in place: how a clip buffer is laid out so
that its frames start at every residue of 16 bytes, the case table ADOPT_L0 -- one small launch for every level-0 kernel that reads a u8
frame, all of widths divisible by 4 (the widths whose quad loads go by the frame's address: raw_quads_aligned, l0_plan.h) plus controls
that load element by element whatever the address -- what klt_level0_path / klt_level0_lean_form must report for each, and a numpy model of
the wrong rule (a device that force-aligns a 4-byte load) with which tests/test_adopt_rule.py shows, without a GPU, that the comparison
of tests/test_gpu_adopt_residues.py would notice it.

The cases are taken from the tables that already exist (pyramid_expected, test_gpu_l0_lean, test_gpu_l0_lean_wave): the smallest case of
each kernel whose width is a multiple of 4, or the smallest one widened to the next multiple.  The path they reach is asked of
expected_path / goes_lean / takes_wave / takes_wide, never restated here."""
import collections
import functools

import numpy as np

import pyramid_expected as pe
import test_gpu_l0_lean as lean_mod
import test_gpu_l0_lean_wave as wave_mod
import test_gpu_l0_wide as wide_mod
from pyramid_expected import Case

GAP_BYTE, GUARD_BYTES, GAP_BYTES = 0x5A, 64, 32
ORACLE_FRAMES = (0, 1, 2, 3)                     # residues 0 .. 3 under the default layout: every class of addr % 4


# ------------------------------------------------------------------------------------------------------------------------------ layout
Layout = collections.namedtuple("Layout", "buf offsets residues size stride")


def pack(frames, residues=None):
    """`n` u8 frames of one size in one buffer: frame k starts at offset k * stride + residues[k] (default k % 16), stride = the frame
    size rounded up to 16, plus 32; every gap holds 0x5A and 64 guard bytes of it come last.  A batch of 32 then has every residue of 16
    twice and every class of addr % 4 eight times, mixed in one launch."""
    n, size = len(frames), frames[0].size
    residues = [k % 16 for k in range(n)] if residues is None else [int(r) for r in residues]
    assert len(residues) == n and all(0 <= r < 16 for r in residues)
    assert all(f.dtype == np.uint8 and f.size == size for f in frames)
    stride = -(-size // 16) * 16 + GAP_BYTES
    offsets = [k * stride + residues[k] for k in range(n)]
    buf = np.full(n * stride + GUARD_BYTES, GAP_BYTE, np.uint8)
    for f, o in zip(frames, offsets):
        assert (buf[o:o + size] == GAP_BYTE).all()
        buf[o:o + size] = f.ravel()
    return Layout(buf, offsets, residues, size, stride)


def addresses(base, layout):
    """the device address of every frame of a layout written at `base`: base on 16 bytes, frames that do not overlap, inside the buffer in
    front of the guard"""
    assert base % 16 == 0, "the buffer must start on 16 bytes for the residues to be the addresses'"
    addr = [base + o for o in layout.offsets]
    assert [a % 16 for a in addr] == layout.residues
    ends = [a + layout.size for a in addr]
    assert all(e <= nxt for e, nxt in zip(ends, addr[1:])) and ends[-1] <= base + layout.buf.size - GUARD_BYTES
    return addr


def force_aligned_frame(layout, k, shape):
    """What a kernel that takes its quad loads' alignment from the width alone computes FROM, on a device that rounds the address of a
    4-byte load down to 4: every quad of a frame whose width is a multiple of 4 comes from addr % 4 bytes further down the buffer (the
    frame before it in memory order: its own bytes shifted, the first ones out of the gap).  Widths that are no multiple of 4 load element
    by element: the frame itself."""
    nrows, ncols = shape
    o, r = layout.offsets[k], layout.offsets[k] % 4
    if ncols % 4:
        r = 0
    return layout.buf[o - r:o - r + layout.size].reshape(nrows, ncols)


# --------------------------------------------------------------------------------------------------------------------------------- cases
# case: the frames and parameters; source: the table the shape was taken from; stream: the KLT_OPT_L0_STREAM value the builds run under;
# lean: None (full builds, KLT_OPT_L0_LAZY_GRAD 0), or the lean form the shape was written for ("banded" / "wave": builds under
# KLT_OPT_L0_LAZY_GRAD 2 with KLT_OPT_L0_LEAN_FORM 0 and 1); no_elision: derivative taps with a centre of -0.0, the one way a u8 frame
# reaches the streaming kernel that keeps the centre product (tests/test_gpu_l0_wide.py)
AdoptCase = collections.namedtuple("AdoptCase", "name case source stream lean no_elision", defaults=(1, None, False))


def _smallest(cases, ok):
    return min((c for c in cases if ok(c)), key=lambda c: (c.ncols * c.nrows * c.batch, c.ncols))


def _quads(c):
    return c.ncols % 4 == 0


def _u8_code(c):
    return pe.case_path(c, False)[0]


def _fused_cases():
    out = []
    take = lambda name, c, source, **kw: out.append(AdoptCase(name, c._replace(table="ADOPT_L0"), source, **kw))
    # the streaming kernel, centre tap elided (what a u8 frame gets) and kept: the two smallest STREAM_* shapes of a width divisible by 4,
    # one segment high and two, 9 and 5 smoothing taps
    elided = _smallest(pe.STREAM_CASES, _quads)
    kept = _smallest(pe.STREAM_CASES, lambda c: _quads(c) and c.sigma != elided.sigma and c.nrows > pe.SEG)
    take("stream-no-centre", elided, "STREAM_CASES")
    take("stream", kept, "STREAM_CASES", no_elision=True)
    # the 32-row tile with the fused reduction: the smallest (one tile column: every tile takes the loop for frames smaller than the halo)
    # and the smallest of two tile columns or more with the other tap count
    hred = _smallest(pe.TILED_HRED_SMALL, lambda c: _quads(c) and _u8_code(c) == pe.RB32_HRED)
    take("rb32-hred-one-column", hred, "TILED_HRED_SMALL")
    take("rb32-hred", _smallest(pe.TILED_HRED_SMALL, lambda c: _quads(c) and _u8_code(c) == pe.RB32_HRED and c.ncols >= 128 and c.sigma != hred.sigma),
         "TILED_HRED_SMALL")
    take("rb32", _smallest(pe.RB32_PLAIN, _quads), "RB32_PLAIN")
    # the 16-row tile: the smallest table case that takes it, and 32 frames just under the bound of the tall tile
    take("rb16", _smallest(pe.ALL_CASES, lambda c: _quads(c) and c.batch <= pe.MAX_BATCH and c.kinds is None and _u8_code(c) == pe.RB16), "MERGED_GRAD")
    take("rb16-below-tall", Case("ADOPT_L0", 248, 126, 0.1), "TILED_HRED_SMALL")
    # seven smoothing taps (smooth_grad_kernel) and the two-pass control: OTHER_PATHS' shape widened to 204, four frames for four residues
    lds, two = pe.OTHER_PATHS
    take("tiled-lds", lds._replace(ncols=-(-lds.ncols // 4) * 4, batch=4), "OTHER_PATHS")
    take("control-two-pass", two._replace(ncols=-(-two.ncols // 4) * 4, batch=4), "OTHER_PATHS")
    # frames smaller than the tile's halo (nc < 128 or nr < 2 tile rows): the tiled kernel's quad-or-element loop
    take("halo-loop-64x48", Case("ADOPT_L0", 64, 48, 0.1, 8, 2, 4), "TILED_HRED_SMALL")
    take("halo-loop-32x64", Case("ADOPT_L0", 32, 64, 0.2, 8, 2, 4), "TILED_HRED_SMALL")
    # controls: widths that are no multiple of 4 load element by element whatever the address
    take("control-stream-mod4-1", _smallest(pe.STREAM_CASES, lambda c: c.ncols % 4 == 1), "STREAM_CASES")
    take("control-tiled-mod4-2", _smallest(pe.TILED_HRED_SMALL, lambda c: c.ncols % 4 == 2 and _u8_code(c) == pe.RB32_HRED), "TILED_HRED_SMALL")
    return out


def _lean_cases():
    out = []
    for geom, (stream, _, _, _) in lean_mod.GEOMETRIES.items():
        _, nc, nr, sigma = min((c for c in lean_mod.CASES if c[0] == geom and c[1] % 4 == 0), key=lambda c: c[1] * c[2])
        out.append(AdoptCase("lean-banded-" + geom, Case("ADOPT_L0", nc, nr, sigma, pe.MAX_BATCH, lean_mod.LEVELS, lean_mod.SS), "lean " + geom, stream, "banded"))
    widths = [c for c in wave_mod.CASES if c[0] == "w"]
    picks = [("whole-last-strip", next(c for c in widths if c[1] == 2 * wave_mod.STRIP)),
             ("4-column-last-strip", next(c for c in widths if c[1] % wave_mod.STRIP == 4)),
             ("height", min((c for c in wave_mod.CASES if c[0] != "w"), key=lambda c: c[1] * c[2]))]
    for name, (_, nc, nr, sigma) in picks:
        assert nc % 4 == 0
        out.append(AdoptCase("lean-wave-" + name, Case("ADOPT_L0", nc, nr, sigma, pe.MAX_BATCH, wave_mod.LEVELS, wave_mod.SS), "lean wave", 2, "wave"))
    return out


ADOPT_L0 = _fused_cases() + _lean_cases()
CONTROLS = [a.name for a in ADOPT_L0 if a.name.startswith("control-")]


def source_pixels(source):
    """pixels per launch of the largest case of the table a case was taken from (its width rounded up to a multiple of 4, as a widened
    case's is)"""
    up4 = lambda nc: -(-nc // 4) * 4
    if source.startswith("lean"):
        geom = source.split()[1]
        shapes = wave_mod.CASES if geom == "wave" else [c for c in lean_mod.CASES if c[0] == geom]
        return max(up4(c[1]) * c[2] * pe.MAX_BATCH for c in shapes)
    return max(up4(c.ncols) * c.nrows * min(c.batch, pe.MAX_BATCH) for c in getattr(pe, source))


def expected(a, lazy=0, form=1):
    """(klt_level0_path code, klt_level0_lean_form) of a build of the case's frames under KLT_OPT_L0_LAZY_GRAD `lazy` (0: full; 2: lean
    wherever a streaming kernel is launched) and KLT_OPT_L0_LEAN_FORM `form`, at the case's own KLT_OPT_L0_STREAM"""
    c = a.case
    ntaps = pe._tap_counts(c.ss, c.sigma)[0]
    wide = a.stream == 2 and c.levels > 1 and c.fused and c.ss == 4 and ntaps in (5, 9) and wide_mod.takes_wide(c.ncols, c.nrows, c.batch)
    if wide:
        code = wide_mod.STREAM_WIDE if a.no_elision else wide_mod.STREAM_WIDE_NO_CENTRE
    else:
        code = pe.expected_path(c.ncols, c.nrows, c.batch, a.no_elision, c.levels, c.ss, c.sigma, stream_opt=min(a.stream, 1), fused_opt=c.fused)[0]
    streams = code in (pe.STREAM, pe.STREAM_NO_CENTRE, wide_mod.STREAM_WIDE, wide_mod.STREAM_WIDE_NO_CENTRE)
    if lazy != 2 or not streams:
        return code, 0
    if a.stream == 2:
        assert wave_mod.goes_lean(c.ncols, c.nrows, c.batch)
    return code, 2 if form == 1 and wave_mod.takes_wave(c.ncols, c.nrows, ntaps) else 1


@functools.lru_cache(maxsize=2)
def case_frames(name):
    (a,) = [a for a in ADOPT_L0 if a.name == name]
    return tuple(pe.case_frames(a.case, False))


def grad_taps(a):
    """None, or the (Gaussian, derivative) gradient taps a case without the centre-tap elision is built with"""
    if not a.no_elision:
        return None
    from pyfeaturetrack_amd.params import taps_from_params
    g, d = taps_from_params(pe.params_from_tc(pe.tc_of(a.case)))[2]
    d = list(d)
    assert d[len(d) // 2] == 0.0
    d[len(d) // 2] = -0.0
    return list(g), d


def oracle_planes(a, frame):
    """[level][plane] of the CPU oracle for one frame of a case (with the case's own gradient taps where it has some: as
    test_gpu_l0_wide.oracle_planes)"""
    from oracle import klt_oracle as ko
    p = pe.oracle_pyramid(a.case, frame)
    out = [[p.level(w, l) for w in range(3)] for l in range(a.case.levels)]
    taps = grad_taps(a)
    if taps is not None:
        g, d = taps
        out = [[img, ko.convolve_separate(img, d, g), ko.convolve_separate(img, g, d)] for img, _, _ in out]
    return out
