"""The level-0 pyramid kernels at the edges of their strips, bands, segments and tiles (the tables of tests/pyramid_expected.py): batches
of 32 small frames reach the streaming kernel and the 32-row tile with the fused first reduction at every class of width and height
remainder.  Every case asserts through klt_level0_path that the kernel it was written for is the one that ran, under the production
configuration (no experiment hook is set), and compares planes bit for bit: no tolerances."""
import pytest

from pyramid_expected import (GROUPING_CASES, STREAM_CASES, STREAM_ORACLE_FRAMES, TILED_CASES, case_id, run_pyramid_trial)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("case", STREAM_CASES, ids=case_id)
def test_stream_case(ctx, case, f32):
    """KLT_OPT_L0_STREAM 1 and 0: the streaming kernel, then the 32-row tile with the reduction (asserted); the three planes of every
    level of ALL frames equal between the two builds; frames 0, 1, 15 and 31 of both equal the oracle's pyramids"""
    bad = run_pyramid_trial(ctx, case, f32, oracle_frames=STREAM_ORACLE_FRAMES)
    assert bad is None, "%s\n%r" % (bad, case)


@pytest.mark.parametrize("f32", [False, True], ids=["u8", "f32"])
@pytest.mark.parametrize("case", TILED_CASES, ids=case_id)
def test_tiled_case(ctx, case, f32):
    """KLT_OPT_FUSED_HREDUCE 1 and 0: the 32-row tile with and without the first reduction (asserted; the launch one pixel short of the
    bound takes 16-row tiles both ways); every level of EVERY frame of both builds equals the oracle's"""
    bad = run_pyramid_trial(ctx, case, f32)
    assert bad is None, "%s\n%r" % (bad, case)


@pytest.mark.parametrize("case", GROUPING_CASES, ids=case_id)
def test_grouping_case(ctx, case):
    """the merged gradient launch at its limits (32 entries, 33 and 34 falling back, three level sizes in one launch), a batch of 33
    split into 32 + 1 (the query reports the last group: 16-row tiles), u8 and f32 frames interleaved (two groups), and the two kernels
    for taps of any count: the path and the merged flag, every frame and every level against the oracle"""
    bad = run_pyramid_trial(ctx, case, False)
    assert bad is None, "%s\n%r" % (bad, case)
