"""The selection score stage at the edges of its tiles, bands and strips (the tables of tests/select_scores_expected.py): the summed-area
tables of sat_rows_pipe / sat_cols_pipe and of the barrier-coupled pair through the eigenvalue map of an unprepared selection, the keys
that klt_select_prepare_async writes -- cols_eigen_pipe where it applies, eigen_hist_kernel elsewhere -- through
klt_download_prepared_keys, all under KLT_OPT_SAT_VARIANT 1 and 0.  Every case asserts through klt_select_score_path that the kernels it
was written for are the ones that ran, and compares with the CPU oracle bit for bit: no tolerances."""
import pytest

from select_scores_expected import (BARRIER, COLS_PIPE, FUSED, ROWS_PIPE, SCORES_SEEDS, SORTED, case_id, draw_scores, run_scores_trial)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _run(ctx, case):
    bad = run_scores_trial(ctx, case)
    assert bad is None, "%s\n%r" % (bad, case)


@pytest.mark.parametrize("case", ROWS_PIPE, ids=case_id)
def test_rows_pipe_case(ctx, case):
    """sat_rows_pipe: 1 .. 7 tiles of 128 columns against its three loaders and three slots, last tiles either side of the half-tile
    split and of the ncols - 2 clamp, bands of 0, 1 and 15 rows read, a frame of 12 rows, odd row counts"""
    _run(ctx, case)


@pytest.mark.parametrize("case", COLS_PIPE, ids=case_id)
def test_cols_pipe_case(ctx, case):
    """sat_cols_pipe: last strips of 64, 4 and 60 columns (the ncols - 4 clamp), 1 .. 7 tiles of 64 rows, row remainders either side of
    a storer's group of four rows"""
    _run(ctx, case)


@pytest.mark.parametrize("case", BARRIER, ids=case_id)
def test_barrier_case(ctx, case):
    """sat_rows_kernel / sat_cols_kernel: tile counts below, at, one above and two turns of their register rings (8 and 12), remainders
    of 1 and 63 columns and of 0, 1 and 31 rows -- as KLT_OPT_SAT_VARIANT 0, and as the fallback of variant 1 on widths that are no
    multiple of 4, which the path code must report"""
    _run(ctx, case)


@pytest.mark.parametrize("case", FUSED, ids=case_id)
def test_fused_case(ctx, case):
    """cols_eigen_pipe: 29, 25, 17 and 9 candidate columns per strip against nx (one strip, remainders 0, 1 and per-strip - 1), 1 .. 9
    tiles of 32 rows, first scored tiles 0, 1 and 2, strips that start at any column mod 4, thresholds pinned to the reference's f64
    compare from both sides; every case twice, with other data behind the rows' ends the second time; and the geometries the kernel
    declines (windows of 25 and 31, skipped pixels), which must report the separate kernels and give the same keys"""
    _run(ctx, case)


@pytest.mark.parametrize("case", SORTED, ids=case_id)
def test_sorted_case(ctx, case):
    """the serial walk's whole sorted candidate list (KLT_OPT_SELECT_PARALLEL_NMS 0) at candidate counts either side of one and two
    2048-key chunks, and of 10 000: the local bitonic sort, the local merge and the global steps at every chunk relation"""
    _run(ctx, case)


@pytest.mark.parametrize("seed", SCORES_SEEDS)
def test_scores_draw(ctx, seed):
    """a drawn path code and a drawn geometry that reaches it (every code occurs in the seed list)"""
    _run(ctx, draw_scores(seed))
