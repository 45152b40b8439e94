"""Gain / bias tracking, per-feature track quality and the motion-model check on seeded random draws (tests/feature_draws_expected.py):
every record of every call equals the numpy restatement of its rule, bit for bit -- val, x, y and the aux word for the tracker, the four
quality fields as bit patterns, every byte of `out` and of the model record for the check.  The tables are fixed;
tests/test_feature_draws_rule.py asserts without a GPU that their entries reach what they claim (every kernel instantiation, both sides
of the four-feature kernel's threshold, the degenerate windows of float32 extremes, both clamps of the correlation, the second trip of
the gather's tile loop, candidate counts on the edges of the look-ahead loops), and tests/fuzz/fuzz_parity.py --light / --quality /
--model runs the same trial functions on fresh seeds."""
import pytest

from feature_draws_expected import (FEATURE_API_SEEDS, LIGHT_SEEDS, MODEL_EDGE_NAMES, MODEL_SEEDS, QUALITY_SEEDS, draw_feature_api, light_case,
                                    model_case, model_edge_case, quality_case, run_feature_api_trial, run_light_trial, run_model_trial,
                                    run_quality_trial)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", LIGHT_SEEDS)
def test_light_draw(ctx, seed):
    """klt_track, a batch of one pair and a batch of 2 - 4 pairs (alternating frame order, a list each) under klt_set_light_params mode 1
    and KLT_OPT_TRACK_VARIANT 0 / 4; klt_track_light_path after every launch"""
    c = light_case(seed)
    bad = run_light_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_quality_draw(ctx, seed):
    """klt_track_quality, n = 1 and klt_track_quality_batch_async of 2 - 4 pairs, twice on one table and once with the pairs reversed"""
    c = quality_case(seed)
    bad = run_quality_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_model_draw(ctx, seed):
    """klt_motion_check on every list and klt_motion_check_batch_async over 2 - 4 lists of equal length"""
    c = model_case(seed)
    bad = run_model_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("name", MODEL_EDGE_NAMES)
def test_model_edge(ctx, name):
    """the fixed table MODEL_EDGES: list lengths around one and two tiles of the gather, tiles without a candidate, candidate counts on
    the edges of the look-ahead loops, frame sizes that set bit 31 of the record's size word, a batch with every outcome"""
    c = model_edge_case(name)
    bad = run_model_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])


@pytest.mark.parametrize("seed", FEATURE_API_SEEDS)
def test_new_features_together_through_the_python_api(seed):
    """tc.lightingCompensation = "gain_bias" on a lit moving-block clip, tc.motionModelCheck = "affine", tc.trackQuality and a selection
    grid (even seeds) or mask (odd seeds) over four frames with KLTReplaceLostFeatures in between"""
    bad = run_feature_api_trial(seed)
    assert bad is None, "%s\n%r" % (bad, draw_feature_api(seed))
