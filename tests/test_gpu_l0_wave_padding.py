"""smooth_grad_lean_wave, the padded LDS rows of a wavefront: a lane reads the quads l - 2 .. l + 2 and the first sample of quad l + 3 of
its row at constant offsets from one address, without a clamp, so lanes 0, 1 and 61 - 63 read two quads of padding left and two quads and
a float of padding right of the 64 quads that the lanes write.  Nothing ever writes the padding: what an earlier workgroup left there is
read, and must reach no stored value (the kernel's header states the invariant: only halo lanes read it, their H1 sample is not
stored).  The raw row's neighbour samples come by a whole-wavefront shift in which lane 0 has no lower and lane 63 no upper neighbour.

Every case builds one batch of 32 distinct frames lean in the wave form, then a batch of OTHER frames of the same shape in the same
context (the LDS of every CU then holds rows of other frames), then the first batch again, and compares, bit for bit and without
tolerances, the compact image plane of level 0 and all three planes of level 1
  * of every frame, second build against first;
  * of frames 0 and 31 against the CPU oracle's (oracle/klt_oracle.py, as tests/test_gpu_l0_lean_wave.py does).

Shapes: those of test_gpu_l0_lean_wave.shapes() at which the reads at the ends of the padded rows differ, with its goes_lean / takes_wave
rules and its batch of 32 frames.  Under goes_lean a batch of 32 goes lean only from 2048 workgroups of a banded geometry on, so a narrow
frame needs many rows and a low frame many columns: as in that module a width comes with the fewest rows that go lean and a height with
the fewest columns (a multiple of 4), not each width with each height.
  * widths 2 x 232 (two whole strips, both at a frame edge), 2 x 232 + 4 (a last strip one quad wide: lanes 4 - 63 are all reflected
    columns), 256 (the smallest width that takes the wave form: a last strip of six quads) and 2 x 232 + 26 (ncols % 4 = 2: element
    loads and predicated stores in every strip);
  * heights 3 SEG - 1 and 2 SEG + 3 (a last segment of SEG - 1 and of 3 rows) on about 4000 columns: interior strips (aligned quad loads) between
    the two edge strips.
u8 and f32 frames; 5 and 9 taps alternate over the shapes and swap between the input types, and the two heights carry different tap
counts: each of the four instantiations runs edge strips (widths) and interior strips (heights)."""
import numpy as np
import pytest

from pyramid_expected import MAX_BATCH, first_difference, frames
from pyfeaturetrack_amd._abi import L0_LEAN_WAVE_COLS as STRIP, L0_LEAN_WAVE_SEG as SEG
from test_gpu_l0_lean_wave import LEVELS, TAPS, WIDTH_MOD4, _build, _fewest, _restore, _setup, goes_lean, oracle_planes, shapes, takes_wave

ORACLE_FRAMES = (0, MAX_BATCH - 1)
SMALLEST = 256                                   # plan_level0: the wave form from 256 columns on


def padding_cases():
    """(kind, ncols, nrows, sigma for u8 frames): four widths, two heights"""
    have = shapes()
    widths = [next(c for c in have if c[0] == "w" and c[1] == nc) for nc in (2 * STRIP, 2 * STRIP + 4)]
    widths.append(("w", SMALLEST, _fewest(lambda nr: goes_lean(SMALLEST, nr), 64), 0.1))
    widths.append(next(c for c in have if c[0] == "w" and c[1] == WIDTH_MOD4[1]))
    heights = [next(c for c in have if c[0] == "h" and c[2] == nr) for nr in (3 * SEG - 1, 2 * SEG + 3)]
    heights[1] = heights[1][:3] + ((0.1, 0.2)[heights[0][3] == 0.1],)           # (the other tap count than the first height's)
    return widths + heights


CASES = padding_cases()


def _sigma(case, f32):
    sigma = case[3]
    return (0.1, 0.2)[sigma == 0.1] if f32 else sigma


def case_id(c):
    return "%s-%dx%d-s%.1f" % c


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _planes(ctx, batch):
    return [[ctx.download_level(k, 0, 0)] + [ctx.download_level(k, p, 1) for p in range(3)] for k in range(batch)]


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_padded_rows_reach_no_stored_value(ctx, case, f32):
    from oracle import klt_oracle as ko
    _, ncols, nrows, _ = case
    sigma = _sigma(case, f32)
    fr = frames((nrows, ncols), MAX_BATCH, f32, ncols * 65536 + nrows + 7)
    other = frames((nrows, ncols), MAX_BATCH, f32, ncols * 65536 + nrows + 8)
    ko.set_threads(8)
    try:
        want = {k: oracle_planes(fr[k], sigma) for k in ORACLE_FRAMES}
    finally:
        ko.set_threads(1)
    _setup(ctx, sigma)
    try:
        _build(ctx, fr, 2, 1, 2)                         # (always lean, the wave form; asserts klt_level0_lean_form = 2)
        first = _planes(ctx, MAX_BATCH)
        _build(ctx, other, 2, 1, 2)
        _build(ctx, fr, 2, 1, 2)
        second = _planes(ctx, MAX_BATCH)
    finally:
        _restore(ctx)
    names = ["image plane of level 0"] + ["plane %d of level 1" % p for p in range(3)]
    for k in range(MAX_BATCH):
        for name, a, b in zip(names, first[k], second[k]):
            bad = first_difference(b, a)
            assert not bad, "frame %d, %s, second build against the first: %s" % (k, name, bad)
    for k in ORACLE_FRAMES:
        for name, got, ref in zip(names, first[k], [want[k][0][0]] + [want[k][1][p] for p in range(3)]):
            bad = first_difference(got, ref)
            assert not bad, "frame %d, %s against the oracle: %s" % (k, name, bad)


# ------------------------------------------------------------------------------------------------------------------------------- no GPU
def test_case_list():
    """the widths and heights the padding is read at, each lean under the host's rule at 32 frames and in the wave form for both tap
    counts; both tap counts at the widths and at the heights for either input type"""
    assert LEVELS == 2
    assert [c[1] for c in CASES[:4]] == [2 * STRIP, 2 * STRIP + 4, SMALLEST, WIDTH_MOD4[1]] and CASES[3][1] % 4 == 2
    assert [c[2] for c in CASES[4:]] == [3 * SEG - 1, 2 * SEG + 3] and all(c[1] % 4 == 0 and c[1] >= 4 * STRIP for c in CASES[4:])
    assert not takes_wave(SMALLEST - 1, CASES[2][2], 5)
    for c in CASES:
        _, nc, nr, _ = c
        assert goes_lean(nc, nr) and not goes_lean(nc, nr, MAX_BATCH - 1), c
        assert takes_wave(nc, nr, 5) and takes_wave(nc, nr, 9), c
        assert nc * nr * MAX_BATCH <= 36000000, c
    for f32 in (False, True):
        assert {TAPS[_sigma(c, f32)] for c in CASES[:4]} == {5, 9} and {TAPS[_sigma(c, f32)] for c in CASES[4:]} == {5, 9}
