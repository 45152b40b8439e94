"""What the minimum-distance tables of tests/select_pick_expected.py cover, asserted without a GPU: every class of tile, cut and loop edge
named there and every value of every field of expected_pick_path; the constants of the restatements against the source lines they restate;
a worked expected_cut for the frame whose histogram sample is blind to what the cut drops; that four wrong restatements of the walk each
change an entry of every table they concern (so the oracle lists the GPU tests compare with can tell them from the right one); and that
every entry's oracle list places a feature unless the entry says otherwise.  These are conditions on the tables, not measurements."""
import pathlib
import re

import numpy as np

import select_pick_expected as sp
from select_pick_expected import ALL_ENTRIES, CUT, PASSES, REPLACE, WALK, REPLACING_SOME, SELECTING_ALL, radius

CSRC = pathlib.Path(__file__).resolve().parent.parent / "pyfeaturetrack_amd" / "csrc"


def _reached(values, wanted, what):
    assert set(wanted) <= set(values), "%s: %s never occur" % (what, sorted(set(wanted) - set(values)))


def _R(e):
    return radius(e.mindist, e.skip)


def test_the_restatements_constants_are_the_sources():
    k = (CSRC / "select_kernels.hip").read_text()
    api = (CSRC / "api_select.hip").read_text()
    m = re.search(r"constexpr int MIS_TILE = (\d+), MIS_CAP = MIS_TILE \* MIS_TILE, MIS_T = (\d+);", k)
    assert (int(m.group(1)), int(m.group(2))) == (sp.MIS_TILE, sp.MIS_T)
    assert int(re.search(r"mis_stage_bytes\(pl\.R\) <= (\d+) \* 1024;", api).group(1)) * 1024 == sp.STAGE_LIMIT
    assert int(re.search(r"j\.by_rank = j\.bound <= (\d+);", api).group(1)) == sp.BOUND_LIMIT
    assert int(re.search(r"g\.ncand > (\d+) && pl\.target < g\.ncand / 2;", api).group(1)) == sp.CAND_LIMIT
    assert int(re.search(r"pl\.target = (\d+)LL \* n;", api).group(1)) == sp.TARGET_PER_SLOT
    assert int(re.search(r"if \(pl\.target < (\d+)\) pl\.target = \1;", api).group(1)) == sp.TARGET_FLOOR
    assert int(re.search(r"constexpr int HIST_BINS = (\d+);", k).group(1)) == sp.HIST_BINS
    assert int(re.search(r"return \(klt_key_bits\(key\) >> (\d+)\) & \(HIST_BINS - 1\);", k).group(1)) == sp.KEY_BIN_SHIFT
    assert int(re.search(r"constexpr int NMS_T = (\d+);", k).group(1)) == sp.NMS_T
    assert int(re.search(r"na\.gw \* na\.gh \* sizeof\(uint32_t\) <= (\d+) \* 1024;", api).group(1)) * 1024 == sp.LDS_GRID_LIMIT
    m = re.search(r"constexpr int RANK_T = (\d+), RANK_GX = (\d+), RANK_GY = (\d+);", k)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (sp.RANK_T, sp.RANK_GX, sp.RANK_GX)
    # the sample of the histogram and the targets in its units
    assert "const bool sampler = a.hist != nullptr && (blockIdx.x & %d) == 0;" % (sp.HIST_SAMPLE - 1) in k
    body = k[k.index("void launch_eigen_hist("):k.index("void launch_mask_hist(")]
    assert "klt_launch(eigen_hist_kernel, dim3(clamp_grid(blocks, %d)), dim3(256), 0, s, a);" % sp.HIST_GRID in body
    assert "sa.hist_target = (unsigned)((j.target + %d) / %d);" % (sp.HIST_SAMPLE - 1, sp.HIST_SAMPLE) in api
    assert "sa.hist_target = %d / %d * j.cut_scale; sa.hist_slots = j.nfill_d; sa.hist_per_slot = %d / %d * j.cut_scale;" % (
        sp.REPLACE_FLOOR, sp.HIST_SAMPLE, sp.REPLACE_PER_SLOT, sp.HIST_SAMPLE) in api
    # the formulas
    assert "return R > 0 ? (W * MIS_TILE + W * W) * sizeof(uint32_t) : 0;" in k and "const size_t W = MIS_TILE + 2 * (R > 0 ? R : 0);" in k
    assert "const int per_side = (MIS_TILE + R) / (R + 1);" in k and "return per_side * per_side < MIS_CAP ? per_side * per_side : MIS_CAP;" in k
    assert "return (a.stage ? mis_stage_bytes(a.R) : 0) + (((size_t)a.acc_cap * sizeof(unsigned short) + 15) & ~(size_t)15);" in k
    assert "j.bound = R < 0 ? ncand : (long long)((nx + R) / (R + 1)) * ((ny + R) / (R + 1));" in api
    assert "pl.R = pl.d >= 0 ? pl.d / g.step : -1;" in api and "return a.R == 9 ? launch_mis_round_t<9>" in k
    assert "ma.sparse = mode == KLT_REPLACING_SOME && pl.prefilter ? 1 : 0;" in api
    # the repeat rests on what mis_init_kernel saw the threshold bin drop, not on the sample's counts
    assert "if (j.filtered && res[1] && info[3]) {" in api and "*a.cut_dropped = 1u;" in k
    # the figures the tables are built around
    assert [sp.tile_capacity(R) for R in (-1, 0, 1, 2, 15, 31, 64)] == [1024, 1024, 256, 121, 4, 1, 1]
    lds = lambda R: sp.stage_bytes(R) + ((sp.tile_capacity(R) * 2 + 15) & ~15)       # noqa: E731
    assert (lds(31), lds(32)) == (47392, 49168) and lds(31) <= 48 * 1024 < lds(32)
    assert sp.stage_bytes(64) == sp.STAGE_LIMIT and sp.stage_bytes(65) > sp.STAGE_LIMIT and sp.stage_bytes(0) == 0
    assert sp.target_of(1024) == 65536 and sp.target_of(1025) == 65600 and sp.target_of(2000) == 128000
    assert sp.bound_of(384, 256, 0) == 98304 == sp.bound_of(384, 256, -1) and sp.bound_of(385, 256, 0) == 98560
    assert sp.walk_grid_in_lds(256, 128, 1) and not sp.walk_grid_in_lds(257, 128, 1)
    assert sp.walk_grid_in_lds(2560, 1280, 10) and not sp.walk_grid_in_lds(2570, 1280, 10)
    assert sp.key_bins(np.float32([1024.0, 1055.75])).tolist() == [4384, 4384] and sp.key_bins(np.float32([1056.0, 2048.0])).tolist() == [4385, 4416]


def test_names_are_unique_and_frames_are_small():
    names = [e.name for e in ALL_ENTRIES] + [w.name for w in WALK]
    assert len(set(names)) == len(names)
    for e in PASSES + REPLACE:
        assert e.nx * e.ny <= 70000 or e.name.startswith(("rank_", "sort_", "tiles4160")), e.name
    for e in CUT:
        nc, nr = sp.frame_dims(e)
        assert nc * nr <= 400000 and (e.nx * e.ny > sp.CAND_LIMIT or e.name == "nocut_512x512"), e.name
    for e in ALL_ENTRIES:
        assert e.walks == (1, 0)                          # every entry under both values of KLT_OPT_SELECT_PARALLEL_NMS


def test_passes_table_radius_and_lattice_classes():
    by_R = {}
    for e in PASSES:
        by_R.setdefault((_R(e), e.skip), []).append(e)
    _reached([R for R, skip in by_R if skip == 0], sp.RADII, "radius")
    for R in sp.RADII:
        es = by_R[R, 0]
        if R > 0:
            assert any(sp.has_interior_tile(e.nx, e.ny, R) for e in es) and any(not sp.has_interior_tile(e.nx, e.ny, R) for e in es), R
            side = sp.MIS_TILE * (2 * -(-R // sp.MIS_TILE) + 1)
            assert sp.has_interior_tile(side, side, R) and not sp.has_interior_tile(sp.MIS_TILE + 2 * R - 1, side, R)
        assert len(es) >= 2
    assert sp.has_interior_tile(160, 160, 64)
    assert {e.mindist for e in by_R[9, 1]} == {19, 20}                                 # R = 9 through nSkippedPixels 1
    # the code paths of mis_round_tile and of the staging loops, and the two walks
    klass = lambda R: ("none" if R <= 0 else "narrow" if R <= 3 else "eight") + ("_c9" if R == 9 else "")       # noqa: E731
    _reached([klass(_R(e)) for e in PASSES], ["none", "narrow", "eight", "eight_c9"], "window loop")
    trips = lambda R: -(-(sp.MIS_TILE + 2 * R) // 64)                                   # noqa: E731
    assert [trips(R) for R in (16, 17, 48, 49)] == [1, 2, 2, 3]
    _reached([trips(_R(e)) for e in PASSES if _R(e) > 0 and sp.parallel_walk(e, 1)], [1, 2, 3], "staging trips of 64")
    assert not sp.parallel_walk(by_R[65, 0][0], 1) and sp.parallel_walk(by_R[64, 0][0], 1)
    _reached([e.nx % 32 for e in PASSES], [0, 1, 31], "nx % 32")
    _reached([e.ny % 32 for e in PASSES], [0, 1, 31], "ny % 32")
    tiles = [np.prod(sp.tiles_of(e.nx, e.ny)) for e in PASSES]
    _reached(tiles, [1, 7, 8, 9, 17], "tile count")
    assert max(tiles) > 4096
    assert any(sp.tiles_of(e.nx, e.ny)[1] == 1 and sp.tiles_of(e.nx, e.ny)[0] > 1 for e in PASSES)      # one tile row
    assert any(sp.tiles_of(e.nx, e.ny)[0] == 1 and sp.tiles_of(e.nx, e.ny)[1] > 1 for e in PASSES)      # one tile column
    for kind in sp.FORMS:
        assert {klass(_R(e)) for e in PASSES if e.form == kind} >= {"narrow", "eight_c9"}, kind
    # ramps: dependency chains far longer than 32 passes, and shorter than the 512 passes the host allows
    chains = [(e.nx if e.form == "rampx" else e.ny) // (_R(e) + 1) for e in PASSES if e.form in ("rampx", "rampy") and _R(e) > 0]
    assert sum(c >= 60 for c in chains) >= 2 and max(chains) <= 200


def test_capacity_entries_fill_full_tiles_exactly():
    seen = set()
    for e in PASSES:
        if e.form != "capacity":
            continue
        R, cap = _R(e), sp.tile_capacity(_R(e))
        seen.add(R)
        out = sp.expected_list(e)
        got = out[out["val"] >= 0]
        tx, ty = ((got["x"] - sp.BORDER) // 32).astype(int), ((got["y"] - sp.BORDER) // 32).astype(int)
        peaks = sp.capacity_peaks(e)
        full = 0
        for j in range(e.ny // 32):
            for i in range(e.nx // 32):
                if peaks[32 * j:32 * j + 32, 32 * i:32 * i + 32].any():
                    full += 1
                    assert int(((tx == i) & (ty == j)).sum()) == cap, (e.name, i, j)
        assert full >= 2, e.name
        assert sp.capacity_tiles_all(R) == (R != 2)
    assert seen == set(sp.CAPACITY_RADII)


def test_value_edges_and_orderings_and_list_lengths():
    edge = [e for e in PASSES if e.form == "edges"]
    assert {e.min_eig for e in edge} == {1.0, 37.5}
    for e in edge:
        val, floor = sp.scores(e), np.float32(e.min_eig)
        for v in (floor, np.nextafter(floor, np.float32(0)), np.float32(1.0), np.float32(sp.BIG)):
            assert (val == v).sum() >= 8, (e.name, v)
        out = sp.expected_list(e)
        assert (out["val"] == 2147483520).any() and int(np.float32(sp.BIG)) == 2147483520 and float(np.nextafter(np.float32(sp.BIG), np.float32(np.inf))) >= 2.0 ** 31
        if e.mindist == 1 and e.n > e.nx * e.ny:                        # nothing excludes anything: every score at the threshold is placed, none below it
            assert int((out["val"] >= 0).sum()) == int((val.astype(np.float64) >= e.min_eig).sum())
            assert (out["val"] == int(e.min_eig)).sum() >= 16
    assert all(np.isfinite(sp.scores(e)).all() for e in PASSES if e.nx * e.ny < 20000)
    # by rank at a bound of 98304, sorted and walked one column further, at R = 0 and R = -1
    order = {(e.nx, _R(e)): sp.expected_pick_path(e, 1)["order"] for e in PASSES if e.name.startswith(("rank_", "sort_"))}
    assert order == {(384, 0): 1, (384, -1): 1, (385, 0): 2, (385, -1): 2}
    # accepted counts against the 96 chunks of mis_rank_kernel, and list lengths against the accepted count
    acc = {e.name: (int(e.form.split(":")[1]), e.n) for e in PASSES if e.name.startswith("accepted_")}
    assert {a for a, n in acc.values()} >= {sp.RANK_GX * sp.RANK_T, sp.RANK_GX * sp.RANK_T + 1, 60000}
    rel = set()
    for e in PASSES:
        if e.name.startswith("accepted_") and e.name != "accepted_none":
            a, n = acc[e.name]
            out = sp.expected_list(e)
            assert int((out["val"] >= 0).sum()) == min(a, n) and int((out["val"] == -1).sum()) == max(n - a, 0), e.name
            rel.add("1" if n == 1 else "a-1" if n == a - 1 else "a" if n == a else "a+1" if n == a + 1 else "4a" if n == 4 * a else "other")
            rel.add(n)
    assert rel >= {"1", "a-1", "a", "a+1", "4a", 255, 256, 257}
    big = [e for e in PASSES if np.prod(sp.tiles_of(e.nx, e.ny)) > 4096]
    assert len(big) == 1 and 0.96 <= float((sp.scores(big[0]) < 1).mean()) <= 0.98


def test_replace_table():
    fixed = [e for e in REPLACE if e.live.startswith("fixed")]
    assert {e.skip for e in fixed} == {0, 1} and {e.live.split(":")[1] for e in fixed} >= {"0", "1", "all"}
    for e in fixed:
        fl, (nc, nr) = sp.list_in(e), sp.frame_dims(e)
        live = fl[fl["val"] >= 0]
        d, step = e.mindist - 1, e.skip + 1
        if e.live.endswith("all"):
            assert live.size == 0
            continue
        assert sp.free_slots(e) == int(e.live.split(":")[1])
        frac = {round(float(v) % 1.0, 2) for v in np.concatenate([live["x"], live["y"]])}
        assert frac >= {0.0, 0.49, 0.5, 0.51}, e.name
        ix, iy = live["x"].astype(int), live["y"].astype(int)
        x_last, y_last = sp.BORDER + (e.nx - 1) * step, sp.BORDER + (e.ny - 1) * step
        assert (ix == sp.BORDER).any() and (ix == x_last).any() and (iy == sp.BORDER).any() and (iy == y_last).any()      # first / last candidate column, row
        assert (ix < d).any() and (ix > nc - 1 - d).any() and (iy < d).any() and (iy > nr - 1 - d).any()                # within d of the frame edge
        assert (ix < sp.BORDER).any() and (ix > x_last).any() and (iy < sp.BORDER).any() and (iy > y_last).any()          # the border margin
        assert (live["x"] >= 0).all() and (live["x"] < nc).all() and (live["y"] >= 0).all() and (live["y"] < nr).all()
        near = (np.abs(ix[:, None] - ix[None, :]) <= 2 * d) & (np.abs(iy[:, None] - iy[None, :]) <= 2 * d)
        assert (near.sum() - live.size) >= 2                                                                             # overlapping squares
        assert sp.live_blocked(e).any() and not sp.live_blocked(e).all()
    long = {e.n: e for e in REPLACE if e.live == "long" and e.mindist == 2}
    assert set(long) == {255, 256, 257, 4095, 4096, 4097, 8193}
    for n, e in long.items():
        lost = np.flatnonzero(sp.list_in(e)["val"] < 0)
        want = sorted({0, n - 1} | {m + k for m in range(256, n, 256) for k in (-1, 0)})
        assert lost.tolist() == want, n
        out = sp.expected_list(e)
        assert (out["val"][lost] >= 0).all()                                                                             # every lost slot is filled
    assert sp.lost_edge_slots(600).tolist() == [0, 255, 256, 511, 512, 599]
    assert any(e.mindist == 0 for e in REPLACE) and any(sp.free_slots(e) > 4096 for e in REPLACE)


def test_cut_table_and_a_worked_blind_sample():
    by = {e.name: e for e in CUT}
    assert not sp.cut_planned(by["nocut_512x512"]) and sp.cut_planned(by["cut_512x513_holds"])
    half = 512 * 513 // 2
    assert [64 * by[k].n - half for k in ("cut_n2051_below_half", "nocut_n2052_at_half", "nocut_n2053_above_half")] == [-64, 0, 64]
    assert [sp.cut_planned(by[k]) for k in ("cut_n2051_below_half", "nocut_n2052_at_half", "nocut_n2053_above_half")] == [True, False, False]
    assert (by["cut_n1024"].n, by["cut_n1025"].n) == (1024, 1025)
    for parallel in (True, False):
        assert sp.cut_of(by["cut_few_valid"], parallel)[1:] == (0, 0)                   # fewer valid keys than the target: no cut
        keys, thr, dropped = sp.cut_of(by["cut_one_bin"], parallel)
        assert (thr, dropped) == (4384, 0) and set(sp.key_bins(keys).ravel().tolist()) == {4384}
    # two bins, exact on the serial walk: the upper one alone is kept from `target` keys on
    two = [sp.cut_of(by["cut_two_bins_target" + k], False)[1:] for k in ("-1", "", "+1")]
    assert two == [(4384, 0), (4416, 512 * 513 - 65536), (4416, 512 * 513 - 65537)]
    plans = [(sp.expected_pick_path(e, w)["attempts"], w, e.mode) for e in CUT if sp.cut_planned(e) for w in (1, 0)]
    assert set(plans) >= {(a, w, SELECTING_ALL) for a in (1, 2) for w in (1, 0)} | {(a, w, REPLACING_SOME) for a in (1, 2) for w in (1, 0)}
    assert sp.expected_pick_path(by["cut_512x513_holds"], 1)["attempts"] == 1 and sp.expected_pick_path(by["cut_runs_out"], 1)["attempts"] == 2
    rep = [e for e in CUT if e.mode == REPLACING_SOME]
    assert {sp.free_slots(e) for e in rep} >= {1, 64, 65, 1000}
    for e in rep:
        tiles = int(np.prod(sp.tiles_of(e.nx, e.ny)))
        assert ((tiles + 7) // 8) % 4 != 0 and sp.expected_pick_path(e, 1)["sparse"] == (sp.expected_pick_path(e, 1)["attempts"] == 1)
    # the worked case: 1024 candidates a row, so the sample -- the 256-key blocks whose index is 0 mod 4 -- is columns 0 .. 255
    e = by["sample_blind"]
    val = sp.scores(e)
    assert (e.nx, e.mindist, e.n) == (1024, 10, 2000) and e.ny >= 300 and sp.target_of(e.n) == 128000 < e.nx * e.ny // 2 == 153600
    assert set(sp.key_bins(val[:, :256]).ravel().tolist()) == {4384} and sp.key_bins(val[:, 256:]).max() < 4384 and val.min() >= 2
    sampled = (np.arange(val.size) // 256 % 4 == 0).reshape(val.shape)
    assert sampled[:, :256].all() and not sampled[:, 256:].any() and int(sampled.sum()) == 256 * e.ny >= 128000 // 4
    assert sp.expected_cut(val, 128000, sampled=True) == (4384, 768 * e.ny)             # the sample: nothing below the bin; in truth three quarters
    thr, dropped = sp.expected_cut(val, 128000, sampled=False)
    assert thr < 4384 and 0 < dropped < 768 * e.ny
    kept = sp.oracle_list(e, np.where(sp.key_bins(val) >= 4384, val, np.float32(0)))
    want = sp.expected_list(e)
    assert int((kept["val"] >= 0).sum()) < 700 and int((want["val"] >= 0).sum()) > 1500      # the left quarter cannot hold the list
    assert int((want["x"] >= sp.BORDER + 256).sum()) > 1000                                # the oracle fills it from the right-hand side
    assert sp.expected_attempts(e, True) == 2 and sp.expected_attempts(e, False) == 2


def test_every_value_of_every_pick_path_field_is_reached():
    runs = [sp.expected_pick_path(e, w) for e in ALL_ENTRIES for w in e.walks]
    assert all(tuple(r) == sp.PICK_FIELDS for r in runs)
    for field, wanted in (("walk", (0, 1)), ("order", (0, 1, 2)), ("cut", (0, 1)), ("attempts", (1, 2)), ("instantiation", (0, 9)), ("grid", (0, 1)),
                          ("sparse", (0, 1))):
        _reached([r[field] for r in runs], wanted, field)
    lds = {r["pass_lds"] for r in runs if r["walk"] == 1}
    assert {2048, 47392, 49168, 122896} <= lds and 0 not in lds and all(r["pass_lds"] == 0 for r in runs if r["walk"] == 0)
    assert any(r["walk"] == 0 for e in PASSES for r in [sp.expected_pick_path(e, 1)])     # the radius too large for the LDS tile, under the parallel option
    draws = [sp.draw_entry(s) for s in sp.DRAW_SEEDS]
    assert draws == [sp.draw_entry(s) for s in sp.DRAW_SEEDS] and len({(d.nx, d.ny, d.mindist, d.form) for d in draws}) >= 10
    assert {d.mode for d in draws} == {SELECTING_ALL, REPLACING_SOME} and len({_R(d) for d in draws}) >= 6
    assert sum(sp.placed_count(d, sp.expected_list(d)) > 0 for d in draws) >= 9


def test_walk_table():
    by = {w.name: w for w in WALK}
    _reached([len(w.keys[0]) for w in WALK], [0, 1, 1023, 1024, 1025, 2049], "nkeys")
    _reached([w.mindist for w in WALK], [0, 1, 2, 3, 7, 11, 100, 255, 256, 257], "mindist")
    assert [sp.walk_grid_in_lds(w.ncols, w.nrows, w.mindist) for w in WALK if w.name.startswith("grid_")] == [True, False, True, False]
    assert max(int(w.keys[1].max()) for w in WALK if len(w.keys[1])) == 65534 == max(int(w.keys[2].max()) for w in WALK if len(w.keys[2]))
    assert {w.n for w in WALK if not w.overwrite} == {1025, 3000} and all(w.live is not None for w in WALK if not w.overwrite)
    # more than 64 survivors in one super-batch, two of them blocked by candidates accepted in it: one in the same 64, one 64 or more before
    w = by["survivors_beyond_lane63"]
    out = sp.walk_expected(w)
    val, x, y = w.keys
    assert len(val) <= sp.NMS_T and int((out["val"] >= 0).sum()) == len(val) - 2 > 64
    placed = {(int(a), int(b)) for a, b in zip(out["x"], out["y"]) if a >= 0}
    blocked = [i for i in range(len(val)) if (int(x[i]), int(y[i])) not in placed]
    assert blocked == [131, 201]
    blockers = [[j for j in range(i) if abs(x[i] - x[j]) <= 9 and abs(y[i] - y[j]) <= 9] for i in blocked]
    assert blockers == [[130], [110]] and 130 // 64 == 131 // 64 and 110 >= 64 and (201 - 1) // 64 > 110 // 64
    # the list fills up on the last key of a super-batch and on the first key of the next
    for name, n in (("full_on_last_key_of_batch", 1024), ("full_on_first_key_of_batch", 1025)):
        w = by[name]
        out = sp.walk_expected(w)
        assert w.n == n and len(w.keys[0]) > n and (out["val"] >= 0).all() and (out["x"][-1], out["y"][-1]) == (w.keys[1][n - 1], w.keys[2][n - 1])
    w = by["mindist0_fewer_slots"]
    assert w.mindist == 0 and w.n < len(w.keys[0])
    for w in WALK:                                       # what klt_min_distance_walk asks of its caller
        val, x, y = w.keys
        assert (val >= 1).all() and (x >= 0).all() and (x < w.ncols).all() and (y >= 0).all() and (y < w.nrows).all() and w.ncols <= 65535 and w.nrows <= 65535
    for w in WALK:                                       # the cases with candidates near each other reject some of them
        if w.name.startswith(("mindist", "grid_")) and w.mindist > 0:
            out = sp.walk_expected(w)
            live = 0 if w.live is None else int((w.live["val"] >= 0).sum())
            assert int((out["val"] >= 0).sum()) - live < min(len(w.keys[0]), w.n - live), w.name


def _changes(entries, mutant):
    """the first of `entries` (smallest lattice first) whose list the wrong restatement changes"""
    for e in sorted(entries, key=lambda e: e.nx * e.ny):
        if e.nx * e.ny > 400000:
            continue
        if sp.lists_difference(sp.walk_restated(e, mutant), sp.expected_list(e)) is not None:
            return e
    return None


def test_the_oracle_lists_tell_four_wrong_walks_from_the_right_one():
    # the right restatement gives the oracle's list
    for e in [PASSES[1], PASSES[9], PASSES[13], REPLACE[0], REPLACE[2], REPLACE[4], REPLACE[9], REPLACE[10], CUT[1], CUT[-1], CUT[-2]] + \
            [e for e in PASSES if e.form in ("edges", "capacity", "ties", "plateau", "checker") and e.nx * e.ny < 20000]:
        assert sp.lists_difference(sp.walk_restated(e), sp.expected_list(e)) is None, e.name
    tied = lambda es: [e for e in es if e.form.split(":")[0] in ("ties", "plateau", "checker", "onebin", "twobins", "blind")]      # noqa: E731
    for table in (PASSES, REPLACE, CUT):
        name = table[0].table
        assert _changes([e for e in table if e.mindist > 1], "strict_square") is not None, name
        assert _changes(tied(table), "ties_left_first") is not None, name
        assert _changes(tied(table), "ties_up_first") is not None, name
        assert _changes(table, "slots_reversed") is not None, name
        assert _changes([e for e in table if e.mode == REPLACING_SOME], "slots_reversed") is not None or table is PASSES, name
    # the walk over a given list: a square one pixel smaller changes a case
    from oracle.min_distance_walk import enforce_minimum_distance
    changed = 0
    for w in WALK:
        if 1 < w.mindist <= 11 and w.live is None:
            val, x, y = w.keys
            pts = [(float(v), int(a), int(b)) for v, a, b in zip(val, x, y)]
            got = enforce_minimum_distance(pts, [[-1, -1, -1] for _ in range(w.n)], w.ncols, w.nrows, w.mindist - 1, 1.0, True)
            want = sp.walk_expected(w)
            changed += [f[0] for f in got] != want["x"].tolist() or [f[1] for f in got] != want["y"].tolist()
    assert changed >= 4


def test_every_entry_places_a_feature_unless_it_says_otherwise():
    for e in ALL_ENTRIES:
        placed = sp.placed_count(e, sp.expected_list(e))
        assert (placed > 0) or e.empty_ok, e.name
        if e.empty_ok and e.table != "DRAW":
            assert placed == 0, e.name


def test_the_list_comparison_notices_one_field_of_one_slot():
    e = PASSES[5]
    want = sp.expected_list(e)
    assert sp.lists_difference(want.copy(), want) is None
    for field, delta in (("x", 1), ("y", -1), ("val", 1)):
        got = want.copy()
        got[field][7] += delta
        assert "1 of %d slots differ; first slot 7" % e.n in sp.lists_difference(got, want)
    assert "shape" in sp.lists_difference(want[1:], want)
