"""What the adopted-frame table of tests/adopt_expected.py covers, asserted without a GPU: the layout puts a frame on every residue of 16
bytes, every level-0 kernel that reads a u8 frame and all three lean forms are some case's expected launch (asked of expected_path,
goes_lean and takes_wave), every case mixes all four classes of addr % 4 in one launch, no case is larger than the table it came from --
and the comparison the GPU tests rest on would notice the wrong rule: on a device that rounds a 4-byte load's address down, a kernel that
takes its quads' alignment from the width alone reads other pixels in every frame that is off 4 bytes."""
import collections

import numpy as np
import pytest

import adopt_expected as ae
import pyramid_expected as pe
import test_gpu_l0_lean as lean_mod
import test_gpu_l0_lean_wave as wave_mod
import test_gpu_l0_wide as wide_mod
from pyramid_expected import expected_path

BY_NAME = {a.name: a for a in ae.ADOPT_L0}


def test_the_layout():
    frames = pe.frames((45, 67), 32, False, 1)                   # 3015 bytes: no multiple of anything
    lay = ae.pack(frames)
    assert lay.stride == 3024 + 32 and lay.buf.size == 32 * lay.stride + 64
    assert lay.residues == [k % 16 for k in range(32)] and lay.offsets == [k * lay.stride + k % 16 for k in range(32)]
    addr = ae.addresses(1 << 21, lay)
    assert collections.Counter(a % 16 for a in addr) == {r: 2 for r in range(16)}
    assert collections.Counter(a % 4 for a in addr) == {r: 8 for r in range(4)}
    covered = np.zeros(lay.buf.size, bool)
    for k, o in enumerate(lay.offsets):
        assert np.array_equal(lay.buf[o:o + lay.size].reshape(45, 67), frames[k]) and not covered[o:o + lay.size].any()
        covered[o:o + lay.size] = True
    assert (lay.buf[~covered] == ae.GAP_BYTE).all() and not covered[-64:].any()
    gaps = [b - (a + lay.size) for a, b in zip(lay.offsets, lay.offsets[1:])]
    assert min(gaps) >= 16                                       # a quad read from addr % 4 bytes further down stays inside the buffer
    with pytest.raises(AssertionError):
        ae.addresses((1 << 21) + 4, lay)
    with pytest.raises(AssertionError):
        ae.pack(frames, residues=[16] * 32)
    other = ae.pack(frames[:5], residues=[1, 2, 3, 5, 15])
    assert [a % 16 for a in ae.addresses(4096, other)] == [1, 2, 3, 5, 15]


def test_every_kernel_that_reads_a_u8_frame_is_some_cases_launch():
    full = {a.name: ae.expected(a)[0] for a in ae.ADOPT_L0 if a.lean is None}
    quads = {n: code for n, code in full.items() if n not in ae.CONTROLS}
    assert all(BY_NAME[n].case.ncols % 4 == 0 for n in quads)
    # the six fused codes of PATH_NAMES (the plain streaming code with u8 frames: derivative taps whose centre is -0.0)
    assert set(quads.values()) == {pe.TILED_LDS, pe.RB16, pe.RB32, pe.RB32_HRED, pe.STREAM, pe.STREAM_NO_CENTRE}
    assert [pe.PATH_NAMES[k] for k in sorted(set(quads.values()))] == pe.PATH_NAMES[1:]
    # ... each asked of expected_path itself, at the case's own parameters
    for n, code in full.items():
        a = BY_NAME[n]
        c = a.case
        assert a.stream == 1 and code == expected_path(c.ncols, c.nrows, c.batch, a.no_elision, c.levels, c.ss, c.sigma, 1, 1, c.fused)[0], n
        assert ae.expected(a, 0, 0) == ae.expected(a, 0, 1) == (code, 0)
    assert [n for n in full if BY_NAME[n].no_elision] == ["stream"] and full["stream"] == pe.STREAM
    # the controls: the two-pass path at 204 x 165, one streaming and one tiled launch of a width that is no multiple of 4
    assert full["control-two-pass"] == pe.TWO_PASS and (BY_NAME["control-two-pass"].case.ncols, BY_NAME["control-two-pass"].case.nrows) == (204, 165)
    assert full["control-stream-mod4-1"] == pe.STREAM_NO_CENTRE and BY_NAME["control-stream-mod4-1"].case.ncols % 4 == 1
    assert full["control-tiled-mod4-2"] == pe.RB32_HRED and BY_NAME["control-tiled-mod4-2"].case.ncols % 4 == 2
    assert (BY_NAME["tiled-lds"].case.ncols, BY_NAME["tiled-lds"].case.nrows) == (204, 165)
    # the shapes the table was to be taken from
    shape = lambda n: (BY_NAME[n].case.ncols, BY_NAME[n].case.nrows)
    assert shape("stream-no-centre") == (4096, 64) and shape("stream") == (2048, 161) and shape("rb32") == (180, 200)
    assert shape("rb32-hred-one-column") == (64, 489) and shape("rb32-hred") in ((200, 160), (196, 160), (196, 191))
    # the tile's loop for frames smaller than its halo: fewer than two tile columns, or fewer than two tile rows
    for n in ("halo-loop-64x48", "halo-loop-32x64", "rb32-hred-one-column"):
        c = BY_NAME[n].case
        rows = 32 if full[n] in (pe.RB32, pe.RB32_HRED) else 16
        assert full[n] in (pe.RB16, pe.RB32, pe.RB32_HRED) and (c.ncols < 2 * 64 or c.nrows < 2 * rows), n
    assert shape("halo-loop-64x48") == (64, 48) and shape("halo-loop-32x64") == (32, 64)


def test_the_16_row_tile_just_under_the_pixel_bound():
    c = BY_NAME["rb16-below-tall"].case
    pixels = c.ncols * c.nrows * c.batch
    assert pe.TALL_PIXELS - 4 * c.nrows * c.batch <= pixels < pe.TALL_PIXELS          # four columns more (the next width of quads) is tall
    assert ae.expected(BY_NAME["rb16-below-tall"])[0] == pe.RB16
    assert expected_path(c.ncols + 4, c.nrows, c.batch, False, c.levels, c.ss, c.sigma)[0] == pe.RB32_HRED


def test_all_three_lean_forms():
    lean = [a for a in ae.ADOPT_L0 if a.lean]
    assert [a.name for a in lean] == ["lean-banded-wide", "lean-banded-narrow", "lean-wave-whole-last-strip", "lean-wave-4-column-last-strip",
                                      "lean-wave-height"]
    forms = set()
    for a in lean:
        c = a.case
        ntaps = wave_mod.TAPS[c.sigma]
        assert c.ncols % 4 == 0 and c.batch == pe.MAX_BATCH and (c.levels, c.ss) == (2, 4)
        code_full, form_full = ae.expected(a, 0, 1)
        assert form_full == 0 and ae.expected(a, 2, 0) == (code_full, 1)
        assert ae.expected(a, 2, 1) == (code_full, 2 if wave_mod.takes_wave(c.ncols, c.nrows, ntaps) else 1)
        forms |= {form_full, ae.expected(a, 2, 0)[1], ae.expected(a, 2, 1)[1]}
        if a.lean == "banded":
            geom = a.name.rsplit("-", 1)[1]
            assert lean_mod.takes_geometry(geom, c.ncols, c.nrows) and a.stream == lean_mod.GEOMETRIES[geom][0]
            assert code_full == lean_mod.GEOMETRIES[geom][3][1]
            assert ("banded",) + (c.ncols, c.nrows, c.sigma) in [("banded",) + s[1:] for s in lean_mod.CASES if s[0] == geom]
            smaller = [s for s in lean_mod.CASES if s[0] == geom and s[1] % 4 == 0 and s[1] * s[2] < c.ncols * c.nrows]
            assert not smaller
        else:
            assert a.stream == 2 and wave_mod.goes_lean(c.ncols, c.nrows) and wave_mod.takes_wave(c.ncols, c.nrows, ntaps)
            assert ae.expected(a, 2, 1)[1] == 2
            assert (c.ncols, c.nrows, c.sigma) in [s[1:] for s in wave_mod.CASES]
            assert code_full == (wide_mod.STREAM_WIDE_NO_CENTRE if wide_mod.takes_wide(c.ncols, c.nrows) else pe.STREAM_NO_CENTRE)
    assert forms == {0, 1, 2}
    widths = {a.name: a.case.ncols for a in lean}
    assert widths["lean-wave-whole-last-strip"] == 2 * wave_mod.STRIP and widths["lean-wave-4-column-last-strip"] % wave_mod.STRIP == 4
    assert BY_NAME["lean-wave-height"].case.nrows % wave_mod.SEG != 0


def test_no_case_is_larger_than_the_table_it_came_from():
    for a in ae.ADOPT_L0:
        c = a.case
        assert c.ncols * c.nrows * c.batch <= ae.source_pixels(a.source), a.name
        assert c.batch <= pe.MAX_BATCH and c.table == "ADOPT_L0"
    assert len(BY_NAME) == len(ae.ADOPT_L0)
    assert sum(a.case.ncols * a.case.nrows * a.case.batch for a in ae.ADOPT_L0) <= 120000000


def test_every_case_mixes_the_four_classes_and_the_comparison_notices_the_wrong_rule():
    """the layout of every case; and the force-align model on every frame of every case: where the width is a multiple of 4, every frame
    that is off 4 bytes is read as other pixels -- in its middle too, which only whole blocks of quads cover -- so its planes cannot equal
    the uploaded frame's; frames on 4 bytes and widths that load element by element are read as they are"""
    assert ae.ORACLE_FRAMES == (0, 1, 2, 3)
    for a in ae.ADOPT_L0:
        c = a.case
        frames = ae.case_frames(a.name)
        assert len(frames) == c.batch and all(f.dtype == np.uint8 and f.shape == (c.nrows, c.ncols) for f in frames)
        lay = ae.pack(frames)
        addr = ae.addresses(1 << 24, lay)
        assert {x % 4 for x in addr} == {0, 1, 2, 3}, a.name
        assert [addr[k] % 4 for k in ae.ORACLE_FRAMES] == [0, 1, 2, 3], a.name
        mid = (slice(c.nrows // 4, -(c.nrows // 4)), slice(c.ncols // 4, -(c.ncols // 4)))
        for k, f in enumerate(frames):
            seen = ae.force_aligned_frame(lay, k, f.shape)
            if addr[k] % 4 == 0 or c.ncols % 4:
                assert np.array_equal(seen, f), (a.name, k)
            else:
                assert (seen[mid] != f[mid]).any() and (seen != f).mean() > 0.5, (a.name, k)
    assert any(a.case.ncols % 4 for a in ae.ADOPT_L0)
