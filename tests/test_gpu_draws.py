"""The forward-backward check, the motion prior and the selection mask on seeded random draws (tests/draws_expected.py): every record of
every call equals the composition made from the CPU oracle alone, bit for bit -- val, x, y and the aux word for the tracker, val, x, y for
the selection.  The tables are fixed; tests/test_draws_rule.py asserts without a GPU that their entries exercise what they claim, and
tests/fuzz/fuzz_parity.py --fb / --guess / --mask runs the same trial functions on fresh seeds.
test_pyramid_draw: the level-0 pyramid kernels on the draws of tests/pyramid_expected.py (the kernel is drawn first, then a frame size and a
batch that reach it), every plane against the oracle bit for bit; tests/test_pyramid_rule.py and fuzz_parity.py --pyramid likewise."""
import pytest

from pyramid_expected import PYRAMID_SEEDS, draw_oracle_frames, drawn_case, run_pyramid_trial
from draws_expected import API_SEEDS, MASK_LARGE_SEEDS, MASK_SEEDS, TRACK_SEEDS, mask_case, run_api_trial, run_mask_trial, run_track_trial, track_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", TRACK_SEEDS)
def test_tracking_draw(ctx, seed):
    """klt_track, klt_track_guess (identity, invalid and drawn guesses), klt_track_fb and klt_track_fb_guess (with and without `back`), and
    the batched forms, under KLT_OPT_TRACK_VARIANT 0 / 4 and KLT_OPT_TRACK_XCD_ORDER 0 / 1"""
    c = track_case(seed)
    bad = run_track_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", MASK_SEEDS)
def test_mask_draw(ctx, seed):
    """the drawn mask as a compact host mask, with a padded stride and as a device mask; selection on unprepared and prepared scores,
    without the prefilter, with the serial walk, and after the mask is cleared"""
    c = mask_case(seed)
    bad = run_mask_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", MASK_LARGE_SEEDS)
def test_mask_draw_above_the_prefilter_threshold(ctx, seed):
    """the same on frames with more than 262144 candidates, the only ones on which the candidate prefilter (mask_hist_kernel) runs and a
    replacement takes the prepared scores"""
    c = mask_case(seed, True)
    bad = run_mask_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", API_SEEDS)
def test_features_together_through_the_python_api(seed):
    """tc.selectionMask (an int32 array holding 256 and -1, a Pillow "1" image, a bool and a uint8 array), tc.forwardBackwardCheck and
    KLTTrackFeatures(guess=KLTPredictConstantVelocity(...)) over four frames with KLTReplaceLostFeatures in between"""
    bad = run_api_trial(seed)
    assert bad is None, bad


@pytest.mark.parametrize("seed", PYRAMID_SEEDS)
def test_pyramid_draw(ctx, seed):
    """a drawn kernel (every klt_level0_path code occurs in the table), merged or separate gradient launches, a drawn batch, dtype, sigma,
    depth and subsampling: the path as expected, the builds with KLT_OPT_L0_STREAM / KLT_OPT_FUSED_HREDUCE on and off equal in every plane
    of every frame, and equal to the oracle"""
    c, f32 = drawn_case(seed)
    bad = run_pyramid_trial(ctx, c, f32, oracle_frames=draw_oracle_frames(c), seed=seed)
    assert bad is None, "%s\n%r f32=%r" % (bad, c, f32)
