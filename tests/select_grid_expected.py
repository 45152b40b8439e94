"""The selection-grid rule (include/klt_gpu.h, klt_set_select_grid) composed from the pinned oracle's own pieces.  A = the candidates
_enforceMinimumDistance accepts, in the order it accepts them, if the list were never full: the oracle's walk over a scratch list with
more free slots than it can fill.  A member is kept iff it is among the first cap(cell) members of A in its cell; the kept members fill
the real list's free slots in list order.  No tolerance anywhere: x, y and val of every record are compared exactly.  Plus the seeded
draws the tests share."""
import functools

import numpy as np

from oracle import klt_oracle as ko
from helpers import make_tc, params_from_tc
from select_mask_expected import KLT_NOT_FOUND, REPLACING_SOME, SELECTING_ALL, frame, rect_mask

__all__ = ["accepted_sequence", "apply_quota", "cells_of", "live_counts", "select_grid_expected", "grid_dims", "draw_grid", "grid_case", "grid_facts",
           "N_DRAWS", "tc_of_grid"]


def grid_dims(ncols, nrows, grid):
    cw, ch, _ = grid
    return -(-ncols // cw), -(-nrows // ch)                    # gw, gh


def cells_of(x, y, ncols, grid):
    """cell index of integer pixel positions"""
    cw, ch, _ = grid
    gw = -(-ncols // cw)
    return (np.asarray(y, np.int64) // ch) * gw + np.asarray(x, np.int64) // cw


def live_counts(fl, ncols, nrows, grid):
    """live(c): records with val >= 0 whose position passes 0 <= x < ncols && 0 <= y < nrows as f32 comparisons (a NaN fails), in the
    cell of ((int)x, (int)y)"""
    gw, gh = grid_dims(ncols, nrows, grid)
    live = np.zeros(gw * gh, np.int64)
    x, y = fl["x"].astype(np.float32), fl["y"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        inside = (fl["val"] >= 0) & (x >= np.float32(0)) & (x < np.float32(ncols)) & (y >= np.float32(0)) & (y < np.float32(nrows))
    np.add.at(live, cells_of(x[inside].astype(np.int64), y[inside].astype(np.int64), ncols, grid), 1)      # (int): truncation
    return live


def apply_quota(A, cap, nslots, ncols, grid):
    """(indices into A of the members that fill the slots, how many members the quota turned away before the slots or A ran out)"""
    cells = cells_of(A["x"].astype(np.int64), A["y"].astype(np.int64), ncols, grid)
    order = np.argsort(cells, kind="stable")                     # members of one cell together, in A's order
    sorted_cells = cells[order]
    first = np.searchsorted(sorted_cells, sorted_cells, side="left")
    nth = np.empty(len(A), np.int64)
    nth[order] = np.arange(len(A)) - first                        # 0 for the first member of A in its cell, 1 for the second, ...
    kept = nth < cap[cells]
    taken = np.nonzero(kept)[0][:nslots]
    walked = len(A) if len(taken) < nslots or nslots == 0 else taken[-1] + 1
    if nslots == 0:
        walked = 0
    return taken, int((~kept[:walked]).sum())


def _candidates(params, img, mask):
    nrows, ncols = img.shape
    bx, by, hw, hh = ko.scan_borders(params)
    skip = params.nSkippedPixels
    if params.smoothBeforeSelecting:
        img = ko.smooth(img, params.smooth_sigma)
    gx, gy = ko.gradients(img, params.grad_sigma)
    val = ko.scan_good_features(gx, gy, bx, by, hw, hh, skip)
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.shape == (nrows, ncols)
        at = mask[by::skip + 1, bx::skip + 1][:val.shape[0], :val.shape[1]]
        val = np.where(at != 0, val, np.float32(0)).astype(np.float32)
    return ko.sorted_candidates(val, ncols, nrows, bx, by, skip), val.shape


def accepted_sequence(params, img, mode=SELECTING_ALL, fl=None, mask=None):
    """A as records (x, y, val), in the order the walk accepts them.  The scratch list: the live records (their squares are marked first,
    KLT_REPLACING_SOME) followed by one free slot more than `bound`, the most candidates that can be pairwise mindist apart -- so some
    slot stays free, which is asserted: the list was never full."""
    img = np.ascontiguousarray(img, np.float32)
    nrows, ncols = img.shape
    cand, (ny, nx) = _candidates(params, img, mask)
    mindist = max(params.mindist, 0)
    per = max(mindist - 1, 0) // (params.nSkippedPixels + 1) + 1       # two accepted candidates differ by `per` lattice steps in x or y
    bound = (-(-nx // per)) * (-(-ny // per))
    live = np.zeros(0, ko.FEAT_DTYPE)
    if mode == REPLACING_SOME:
        live = np.array(fl, ko.FEAT_DTYPE)
        live = live[live["val"] >= 0]
    scratch = np.concatenate([live, ko.make_featurelist(bound + 1)])
    ko.enforce_min_distance(cand, scratch, ncols, nrows, mindist, params.min_eigenvalue, mode == SELECTING_ALL)
    free = scratch[len(live):]
    accepted = free["val"] >= 0
    assert not accepted.all(), "the scratch list filled: A may be longer"
    count = int(accepted.sum())
    assert accepted[:count].all()
    return free[:count].copy()


def select_grid_expected(params, img, n, grid, mode=SELECTING_ALL, fl=None, mask=None, A=None):
    """records of the selection on `img` under `grid` = (cell_width, cell_height, max_per_cell); `fl`: the list a KLT_REPLACING_SOME
    selection starts from (not modified); `A`: accepted_sequence of the same arguments, when the caller has it"""
    img = np.ascontiguousarray(img, np.float32)
    nrows, ncols = img.shape
    if A is None:
        A = accepted_sequence(params, img, mode, fl, mask)
    out = ko.make_featurelist(n) if fl is None or mode == SELECTING_ALL else np.array(fl, ko.FEAT_DTYPE)
    gw, gh = grid_dims(ncols, nrows, grid)
    cap = np.full(gw * gh, grid[2], np.int64)
    if mode == REPLACING_SOME:
        cap = np.maximum(cap - live_counts(out, ncols, nrows, grid), 0)
        slots = np.nonzero(out["val"] < 0)[0]
    else:
        slots = np.arange(n)
    taken, _ = apply_quota(A, cap, len(slots), ncols, grid)
    k = len(taken)
    out[slots[:k]] = A[taken]
    if mode == SELECTING_ALL:                                    # the slots the members did not reach
        rest = slots[k:]
        out["x"][rest], out["y"][rest], out["val"][rest], out["aux"][rest] = -1.0, -1.0, KLT_NOT_FOUND, 0
    return out


# ---- seeded draws: size, window, borders, mindist, nSkippedPixels, cells, q, n, mode, mask or none
N_DRAWS = 16


def draw_grid(k):
    """draw k of N_DRAWS.  What the table must cover is dealt round, the rest is drawn: both modes; mindist 0 and 1 among others;
    nSkippedPixels > 0; cells that do not divide the frame; small and large max_per_cell (capped and uncapped cells), short and long
    lists (full and not full)"""
    rng = np.random.default_rng([int(k), 9])
    t = dict(k=int(k), window=int(rng.choice([3, 5, 7, 9])), mode=[SELECTING_ALL, REPLACING_SOME][k % 2],
             mindist=[10, 0, 1, 5, 14, 1, 0, 7][k % 8], skip=[0, 0, 1, 0, 2, 0, 0, 1][(k // 2) % 8])
    t["border"] = None if rng.random() < 0.6 else int(rng.integers(t["window"] // 2 + 1, 30))
    t["w"], t["h"] = int(rng.integers(97, 260)), int(rng.integers(83, 200))
    t["cw"], t["ch"] = int(rng.integers(9, t["w"] // 2)), int(rng.integers(9, t["h"] // 2))
    if k % 5 == 4:
        t["cw"] = t["w"] + int(rng.integers(0, 50))             # one cell column
    t["q"] = int([1, 2, 3, 70, 5, 1000][k % 6])                  # 70: beyond the filter's rounds; 1000: never reached
    t["n"] = int([20, 60, 150, 400][(k // 3) % 4])
    t["lost_share"] = float(rng.choice([0.1, 0.3, 0.6]))
    t["masked"] = bool(k % 4 == 3)
    t["texture"] = int(rng.integers(0, 1 << 30))
    return t


def tc_of_grid(t):
    tc = make_tc(window=t["window"], mindist=t["mindist"], nSkippedPixels=t["skip"])
    if t["border"] is not None:
        tc.borderx = tc.bordery = t["border"]
    return tc


@functools.lru_cache(maxsize=None)
def grid_case(k):
    """a draw's inputs and expected lists (oracle alone, never modified)"""
    t = draw_grid(k)
    tc = tc_of_grid(t)
    p = params_from_tc(tc)
    f = frame(t["w"], t["h"], seed=t["texture"])
    img = f.astype(np.float32)
    grid = (t["cw"], t["ch"], t["q"])
    mask = rect_mask(t["w"], t["h"]) if t["masked"] else None
    start = None
    if t["mode"] == REPLACING_SOME:                              # the plain selection with a drawn share lost
        start = ko.select_good_features(p, img, t["n"])
        lost = np.random.default_rng([int(k), 10]).random(t["n"]) < t["lost_share"]
        start["x"][lost], start["y"][lost], start["val"][lost] = -1.0, -1.0, KLT_NOT_FOUND
    A = accepted_sequence(p, img, t["mode"], start, mask)
    want = select_grid_expected(p, img, t["n"], grid, t["mode"], start, mask, A)
    c = dict(t=t, tc=tc, p=p, frame=f, grid=grid, mask=mask, start=start, A=A, want=want)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def grid_facts(c):
    """what a draw reaches"""
    t, want, start, A, grid = c["t"], c["want"], c["start"], c["A"], c["grid"]
    w, h = t["w"], t["h"]
    free = np.ones(t["n"], bool) if start is None else start["val"] < 0
    placed = free & (want["val"] >= 0)
    held = live_counts(want, w, h, grid)
    before = live_counts(start, w, h, grid) if start is not None and t["mode"] == REPLACING_SOME else np.zeros_like(held)
    full = bool(placed.sum() == free.sum())
    _, turned_away = apply_quota(A, np.maximum(grid[2] - before, 0), int(free.sum()), w, grid)
    return dict(full=full, capped=turned_away > 0, turned_away=turned_away, uncapped=bool((held < grid[2]).any()), partial=bool(w % grid[0] or h % grid[1]),
                placed=int(placed.sum()), free=int(free.sum()), members=len(A))
