"""The epipolar check, the homography check and the crowding check on seeded random draws and on fixed edge tables
(tests/check_draws_expected.py): every record of every call equals the restatement of its rule, byte for byte -- `out`, the model record
or the crowd records, and the count of flagged records.  The tables are fixed; tests/test_check_draws_rule.py asserts without a GPU that
their entries reach what they claim (a refit that fails: valid 2; the strided argmax above 512 hypotheses; candidate counts on the edges of
the three look-ahead loops; the second trip of the gather in batched form; every branch of null9's pivot search; the crowding check's
cell sides, scan classes and the resolve kernel without LDS states in a batch), and tests/fuzz/fuzz_parity.py --epipolar / --homography /
--crowd runs the same trial functions on fresh seeds."""
import numpy as np
import pytest

from check_draws_expected import (CROWD_EDGE_NAMES, CROWD_SEEDS, EPIPOLAR_EDGE_NAMES, EPIPOLAR_SEEDS, HOMOGRAPHY_EDGE_NAMES, HOMOGRAPHY_SEEDS, RULES,
                                  consensus_case, consensus_edge_case, crowd_case, crowd_edge_case, crowd_differ, run_consensus_trial, run_crowd_trial)
from feature_draws_expected import model_differ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _consensus(ctx, c):
    bad = run_consensus_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])
    rule = RULES[c["rule"]]
    assert getattr(ctx, rule.name + "_check_path")() == 2                  # the trial's last launch is the batch
    fin, fout, want = c["pairs"][0], c["pairs"][1], c["want_out"][0]
    _, _, flagged = getattr(ctx, rule.name + "_check")(fin, fout)
    assert getattr(ctx, rule.name + "_check_path")() == 1
    assert flagged == int((want["val"] == rule.outlier).sum()) - int((fout["val"] == rule.outlier).sum())


def _crowd(ctx, c):
    bad = run_crowd_trial(ctx, c)
    assert bad is None, "%s\n%r" % (bad, c["t"])
    assert ctx.crowd_check_path() == 2
    _, _, flagged = ctx.crowd_check(c["outs"][0], c["prevs"][0])
    assert ctx.crowd_check_path() == 1 and flagged == int((c["want_crowd"][0]["val"] == 2).sum())


@pytest.mark.parametrize("name", EPIPOLAR_EDGE_NAMES)
def test_epipolar_edge(ctx, name):
    """the fixed table EPIPOLAR_EDGES: every list alone through klt_epipolar_check, then the lists as one klt_epipolar_check_batch_async"""
    _consensus(ctx, consensus_edge_case("epipolar", name))


@pytest.mark.parametrize("seed", EPIPOLAR_SEEDS)
def test_epipolar_draw(ctx, seed):
    _consensus(ctx, consensus_case("epipolar", seed))


@pytest.mark.parametrize("name", HOMOGRAPHY_EDGE_NAMES)
def test_homography_edge(ctx, name):
    """the fixed table HOMOGRAPHY_EDGES: every list alone through klt_homography_check, then the lists as one batch"""
    _consensus(ctx, consensus_edge_case("homography", name))


@pytest.mark.parametrize("seed", HOMOGRAPHY_SEEDS)
def test_homography_draw(ctx, seed):
    _consensus(ctx, consensus_case("homography", seed))


@pytest.mark.parametrize("name", CROWD_EDGE_NAMES)
def test_crowd_edge(ctx, name):
    """the fixed table CROWD_EDGES: every list alone with and without its previous step, then the lists as one klt_crowd_check_batch_async"""
    _crowd(ctx, crowd_edge_case(name))


@pytest.mark.parametrize("seed", CROWD_SEEDS)
def test_crowd_draw(ctx, seed):
    _crowd(ctx, crowd_case(seed))


def test_the_four_checks_in_turn_keep_their_own_records(ctx):
    """the motion-model, the epipolar, the homography and the crowding check in turn on one context, each into buffers of its own, over
    the two valid-2 lists and a list of 2049 candidates: every check equals its rule, and after each call the records the other checks
    wrote before are unchanged (they share launches and the context, not their scratch)"""
    from crowd_expected import crowd_check_expected
    from model_expected import MODEL_DTYPE, motion_check_expected
    ee, eh = consensus_edge_case("epipolar", "valid2"), consensus_edge_case("homography", "valid2")
    em = consensus_edge_case("epipolar", "m2049")
    IN, OUT, M_REC, E_REC, H_REC, K_OUT, K_REC = 600, 601, 602, 603, 604, 605, 606
    for c in (ee, eh, em):
        t, fin, fout = c["t"], c["pairs"][0], c["pairs"][1]
        n, size = len(fin), dict(ncols=t["ncols"], nrows=t["nrows"])
        kw = dict(t["params"], min_inliers=max(8, t["params"]["min_inliers"]))
        mkw = dict(kw, min_area=0.0)
        ctx.set_model_params(**size, **mkw)
        ctx.set_epipolar_params(**size, **kw)
        ctx.set_homography_params(**size, **kw)
        ctx.set_crowd_params(**size, min_distance=3)
        want = {"model": motion_check_expected(fin, fout, t["ncols"], t["nrows"], **mkw),
                "epipolar": RULES["epipolar"].mod.epipolar_check_expected(fin, fout, t["ncols"], t["nrows"], **kw),
                "homography": RULES["homography"].mod.homography_check_expected(fin, fout, t["ncols"], t["nrows"], **kw)}
        want_crowd = crowd_check_expected(fout, None, t["ncols"], t["nrows"], 3)
        dtypes = {"model": MODEL_DTYPE, "epipolar": RULES["epipolar"].dtype, "homography": RULES["homography"].dtype}
        recs = {"model": M_REC, "epipolar": E_REC, "homography": H_REC}
        down = {"model": ctx.model_download, "epipolar": ctx.epipolar_download, "homography": ctx.homography_download}
        launch = {"model": ctx.motion_check_async, "epipolar": ctx.epipolar_check_async, "homography": ctx.homography_check_async}
        ctx.featbuf_upload(IN, fin)
        done = []

        def others_unchanged(after):
            for name in (k for k in done if k != "crowd"):
                got = np.asarray(down[name](recs[name]), dtypes[name]).reshape(1)
                assert got.tobytes() == np.asarray(want[name][1], dtypes[name]).reshape(1).tobytes(), "%s's record after %s" % (name, after)
            if "crowd" in done:
                assert crowd_differ(ctx.featbuf_download(K_OUT, n), ctx.crowd_download(K_REC, n), want_crowd[0], want_crowd[1], "crowd after " + after) is None

        for _ in range(2):
            for name in ("model", "epipolar", "homography"):
                ctx.featbuf_upload(OUT, fout)
                launch[name](IN, OUT, recs[name], n)
                bad = model_differ(ctx.featbuf_download(OUT, n), down[name](recs[name]), want[name][0], want[name][1], name, dtypes[name])
                assert bad is None, bad
                if name not in done:
                    done.append(name)
                others_unchanged(name)
            ctx.featbuf_upload(K_OUT, fout)
            ctx.crowd_check_async(K_OUT, -1, K_REC, n)
            if "crowd" not in done:
                done.append("crowd")
            others_unchanged("crowd")
        if c is not em:
            assert want[c["rule"]][1]["valid"] == 2
        print("%s: valid model %d, epipolar %d, homography %d; %d crowded" % (t["name"], want["model"][1]["valid"], want["epipolar"][1]["valid"],
                                                                             want["homography"][1]["valid"], (want_crowd[1]["val"] == 2).sum()))
    ctx.set_model_params(mode=0)
    ctx.set_epipolar_params(mode=0)
    ctx.set_homography_params(mode=0)
    ctx.set_crowd_params(mode=0)
