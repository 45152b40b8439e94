"""The edge tables of the two ingest stages (tests/ingest_edges_expected.py) without a device: every class of the kernels' loops and
32-bit bounds is reached by a named entry (printed: tests/COVERAGE.md quotes it), the banded evaluation of the CLAHE rule equals the
unbanded one, the constants the class functions mirror are the sources', the bound shapes are on the sides of 2^32 the table says, and
every wrong restatement of a rule changes the expected bytes of a named entry."""
import pathlib
import re

import numpy as np
import pytest

import equalize_expected as ee
import ingest_edges_expected as ie
import remap_expected as re_

CSRC = pathlib.Path(__file__).resolve().parent.parent / "pyfeaturetrack_amd" / "csrc"
# the shape table of tests/test_equalize_rule.py (that of tests/test_gpu_equalize.py and the golden frame's size)
SHAPES = [(64, 48, 8, 8, 768), (67, 45, 3, 2, 768), (33, 17, 4, 3, 1), (5, 3, 5, 3, 768), (4, 4, 1, 1, 0), (130, 70, 64, 64, 768),
          (320, 240, 8, 8, 768), (320, 240, 8, 8, 10240)]


# ------------------------------------------------------------------------------------------------------------------- constants
def test_the_kernels_constants_are_the_sources():
    eq = (CSRC / "equalize_kernels.hip").read_text()
    for name, value in (("LUT_THREADS", ie.LUT_THREADS), ("HIST_COPIES", ie.HIST_COPIES), ("APPLY_THREADS", ie.APPLY_THREADS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, eq).group(1)) == value
    assert "for (int it = tid; it < items; it += LUT_THREADS) {" in eq and "for (int it = tid; it < items; it += APPLY_THREADS) {" in eq
    assert eq.count("const int per_row = (w + 30) >> 4, items = per_row * h;") == 1
    assert eq.count("const int per_row = (nc + 30) >> 4, items = per_row * (yb - ya);") == 1
    assert "for (int i = tid; i < Tx * 16; i += APPLY_THREADS) {" in eq
    assert "const int t = (int)((((unsigned)xs + 1u) * (unsigned)Tx - 1u) / (unsigned)nc);" in eq
    api = (CSRC / "api_frames.hip").read_text()
    rule = (CSRC / "ingest_rule.h").read_text()                  # (the host rules of the ingest path; api_frames.hip launches by them)
    body = rule[rule.index("inline int eq_apply_split"):rule.index("// ---- grouping")]
    assert "const int split = (%d + bands * batch - 1) / (bands * batch);" % ie.SPLIT_TARGET in body
    assert "const int most = std::max(1, nrows / tiles_y / %d);" % ie.SPLIT_ROWS in body
    assert "return std::max(1, std::min(split, most));" in body and "const int bands = tiles_y + 1;" in body
    assert api.count("a.split = eq_apply_split(nr, a.tiles_y, batch);") == 1
    rm = (CSRC / "remap_kernels.hip").read_text()
    assert int(re.search(r"constexpr int PIECE = (\d+);", rm).group(1)) == ie.PIECE
    assert int(re.search(r"constexpr int PIECES_ACROSS = (\d+);", rm).group(1)) == ie.PIECES_ACROSS
    assert int(re.search(r"constexpr int WAVE_ROWS = \d+, GROUP_ROWS = (\d+);", rm).group(1)) == ie.GROUP_ROWS
    assert "const int per_row = (a.ncols + 2 * (PIECE - 1)) / PIECE;" in rm and "if (a.ncols >= 2) klt_launch(remap_kernel<true>" in rm
    assert int(re.search(r"constexpr int KLT_MAX_BATCH = (\d+);", (CSRC / "l0_plan.h").read_text()).group(1)) == ie.MAX_BATCH
    assert "T group[KLT_MAX_BATCH];" in rule and "i < n && count < KLT_MAX_BATCH; i++)" in rule
    assert api.count("return a.first == b.first && same_size(a.second, b.second);") == 1    # the stages' launches: one stage, one size
    # the split of the shapes the table is built around
    assert ie.clahe_split(1025, 1) == (256, "rows") and ie.clahe_split(2049, 1) == (512, "1024") and ie.clahe_split(1080, 8) == (33, "rows")
    assert ie.clahe_split(36, 2) == (4, "rows") and ie.clahe_split(65535, 64) == (16, "1024")


def test_an_empty_band_never_meets_a_split():
    """a band of zero rows is the one above the first centre of a first tile ONE row high; `most` is then 1 and so is the split"""
    for tiles_y in range(1, 65):
        for nrows in list(range(tiles_y, tiles_y + 200)) + [4200, 65535]:
            cy = ie._centres(nrows, tiles_y)
            rows = np.diff(np.concatenate([[0], cy >> 1, [nrows]]))
            assert (rows[1:] > 0).all()
            if rows[0] == 0:
                assert nrows // tiles_y == 1 and ie.clahe_split(nrows, tiles_y)[0] == 1


# ------------------------------------------------------------------------------------------------------------- the banded rule
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d_%d" % s)
def test_banded_clahe_equals_the_unbanded_one(shape):
    ncols, nrows, tx, ty, clip_q8 = shape
    for frame in (ee.random_frame(ncols, nrows, 3), ee.constant_frame(ncols, nrows), ee.two_bin_frame(ncols, nrows), ie.noise_frame(ncols, nrows, 9)):
        want = ee.clahe(frame, tx, ty, clip_q8)
        for band in (None, ie.BAND, 7):
            assert np.array_equal(ie.clahe(frame, tx, ty, clip_q8, band=band), want), band


def test_remap_copy_equals_the_rule():
    for seed in range(6):
        frame, (mx, my), _, _ = re_.trial(seed)
        assert np.array_equal(ie.remap(frame, mx, my), re_.remap(frame, mx, my))


# ----------------------------------------------------------------------------------------------------------------- CLAHE classes
@pytest.fixture(scope="module")
def clahe_table():
    return {name: ie.clahe_classes(case, ie.clahe_reference(name)[1]) for name, case in ie.CLAHE_EDGES.items()}


# class -> (what must hold of an entry's classes, the entries that must reach it)
CLAHE_CLASSES = {
    "LUT loop: one trip of exactly 1024 items": (lambda c: c["lut_items"] == 1024, ["lut_1x1024_p1", "extent_1x65535_1x64"]),
    "LUT loop: a second trip of ONE piece": (lambda c: c["lut_items"] == 1025, ["lut_1x1025_p1", "lut_1x1025_p2", "lut_1x1025_p14"]),
    "LUT loop: three trips": (lambda c: c["lut_trips"] == 3, ["lut_16x1025_p16", "real_1920x1080_random"]),
    "LUT loop: five trips": (lambda c: c["lut_trips"] == 5, ["lut_16x2049_p16"]),
    "LUT loop: more than 250 trips": (lambda c: c["lut_trips"] > 250, list(ie.LARGE_ENTRIES)),
    "a bin of exactly 2^16": (lambda c: c["largest_bin"] == 1 << 16, ["count_256x256_constant_c0"]),
    "a bin above 2^16": (lambda c: c["largest_bin"] > 1 << 16, ["count_256x257_constant_c768", "large_c_4096x4200_1x1_noise"]),
    "a bin above 2^24": (lambda c: c["largest_bin"] > 1 << 24, ["large_c_4096x4200_1x1_constant"]),
    "a tile of 2^16 pixels and more": (lambda c: c["largest_area"] >= 1 << 16, ["count_256x256_constant_c0", "count_256x257_two_bin_c768"]),
    "a tile of 2^24 pixels and more": (lambda c: c["largest_area"] >= 1 << 24, ["large_c_4096x4200_1x1_noise"]),
    "cap 1 through max(1, 0)": (lambda c: False, []),                                   # (filled in below: needs the case)
    "excess at and above 2^16": (lambda c: any(e >= 1 << 16 for _, e, _, _ in c["clip"]), ["count_256x257_constant_c1", "large_c_4096x4200_1x1_constant"]),
    "excess >> 8 at and above 256": (lambda c: any(s >= 256 for _, _, s, _ in c["clip"]), ["count_256x257_constant_c1"]),
    "excess % 256 of 0, excess > 0": (lambda c: any(e > 0 and r == 0 for _, e, _, r in c["clip"]), ["redist_16x17_r0", "count_256x256_constant_c768"]),
    "excess % 256 of 1": (lambda c: any(r == 1 for _, _, _, r in c["clip"]), ["redist_16x17_r1"]),
    "excess % 256 of 255": (lambda c: any(r == 255 for _, _, _, r in c["clip"]), ["redist_16x17_r255", "count_256x257_constant_c1"]),
    "excess % 256 of another value": (lambda c: any(1 < r < 255 for _, _, _, r in c["clip"]), ["redist_16x17_r15", "redist_67x45_3x2_two_bin"]),
    "clip on, no bin above the cap": (lambda c: any(cap > 0 and e == 0 for cap, e, _, _ in c["clip"]), ["redist_16x17_no_excess"]),
    "clip off": (lambda c: all(cap == 0 for cap, _, _, _ in c["clip"]), ["count_256x257_constant_c0"]),
    "clip_q8 * A at and above 2^32": (lambda c: c["clip_product_64bit"], ["count_256x257_constant_c1048576", "lut_16x1025_clip_2_20"]),
    "LUT numerator at and above 2^32": (lambda c: c["numerator_64bit"], ["large_c_4096x4200_1x1_noise", "large_c_4096x4200_1x1_constant"]),
    "all 16 values of mis": (lambda c: c["mis"] == list(range(16)), ["lut_1x1024_p1", "lut_16x1025_p17", "lut_16x2049_p29", "extent_1x65535_1x64"]),
    "split set by the 1024 bound": (lambda c: c["split_bound"] == "1024" and c["split"] > 1, ["lut_16x2049_p16", "extent_1x65535_1x64"]),
    "split set by the rows": (lambda c: c["split_bound"] == "rows" and c["split"] > 1, ["lut_16x1025_p16", "real_1920x1080_random", "apply_1040x36_1x2"]),
    "split 1": (lambda c: c["split"] == 1, ["apply_40x5_rows_are_tiles"]),
    "apply loop: one trip": (lambda c: c["apply_trips"] == 1, ["apply_130x20_tx2"]),
    "apply loop: two trips": (lambda c: c["apply_trips"] == 2, ["apply_1040x36_1x2"]),
    "apply loop: three trips and more": (lambda c: c["apply_trips"] >= 3, ["real_1920x1080_random", "extent_65535x1_64x1"]),
    "a band of zero rows": (lambda c: c["empty_bands"] > 0, ["apply_40x5_rows_are_tiles", "extent_65535x1_64x1"]),
    "tiles_x below 16": (lambda c: c["tiles_x_class"] == "below 16", ["apply_130x20_tx1", "apply_130x20_tx2"]),
    "tiles_x 16": (lambda c: c["tiles_x_class"] == "16", ["apply_130x20_tx16"]),
    "tiles_x above 16, LUT copy in two trips": (lambda c: c["lut_copy_trips"] == 2, ["apply_130x20_tx17"]),
    "tiles_x 64, LUT copy in four trips": (lambda c: c["lut_copy_trips"] == 4, ["apply_130x20_tx64", "apply_64x9_one_pixel_tiles"]),
    "a piece without a centre": (lambda c: 0 in c["centres_per_piece"], ["real_1920x1080_random"]),
    "a piece across one centre": (lambda c: 1 in c["centres_per_piece"], ["real_1920x1080_random"]),
    "a piece across two centres and more": (lambda c: 2 in c["centres_per_piece"], ["apply_130x20_tx16", "apply_64x9_one_pixel_tiles"]),
    "a piece's first pixel left of its tile's centre": (lambda c: "left" in c["first_pixel_side"], ["apply_130x20_tx2"]),
    "a piece's first pixel right of its tile's centre": (lambda c: "right" in c["first_pixel_side"], ["apply_130x20_tx2"]),
    "Dx * Dy * 255 within 65536 of 2^32": (lambda c: (1 << 32) - 65536 <= c["dxdy255"] < 1 << 32, ["large_a_4096x4112_2x2"]),
    "a single product at and above 2^31": (lambda c: c["single_product"] >= 1 << 31, ["large_a_4096x4112_2x2"]),
    "D of 1 on the x axis alone": (lambda c: False, []),
    "D of 1 on the y axis alone": (lambda c: False, []),
    "remainder at the turn, even D": (lambda c: "at the turn, even D" in c["rounding"], ["apply_130x20_tx2", "real_1920x1080_random"]),
    "remainder at the turn, odd D": (lambda c: "at the turn, odd D" in c["rounding"], ["apply_130x20_tx16", "redist_67x45_3x2_two_bin"]),
    "remainder below the turn, even D": (lambda c: "below the turn, even D" in c["rounding"], ["real_1920x1080_random"]),
    "remainder below the turn, odd D": (lambda c: "below the turn, odd D" in c["rounding"], ["apply_130x20_tx2"]),
}


def test_the_clahe_table_reaches_every_class(clahe_table):
    by_case = {
        "cap 1 through max(1, 0)": lambda n: ie.CLAHE_EDGES[n].clip_q8 > 0 and (ie.CLAHE_EDGES[n].clip_q8 * clahe_table[n]["largest_area"]) >> 16 == 0,
        "D of 1 on the x axis alone": lambda n: ie.CLAHE_EDGES[n].tiles_x == 1 and ie.CLAHE_EDGES[n].tiles_y > 1,
        "D of 1 on the y axis alone": lambda n: ie.CLAHE_EDGES[n].tiles_y == 1 and ie.CLAHE_EDGES[n].tiles_x > 1,
    }
    named = {"cap 1 through max(1, 0)": ["redist_16x17_cap_from_max", "apply_130x20_tx64"],
             "D of 1 on the x axis alone": ["large_d_4096x4200_1x2", "apply_1040x36_1x2"], "D of 1 on the y axis alone": ["large_d_4096x4200_2x1", "extent_65535x1_64x1"]}
    for what, (holds, must) in CLAHE_CLASSES.items():
        if what in by_case:
            reached, must = [n for n in clahe_table if by_case[what](n)], named[what]
        else:
            reached = [n for n, c in clahe_table.items() if holds(c)]
        print("%s: %s" % (what, ", ".join(reached)))
        assert reached and set(must) <= set(reached), (what, must, reached)
    for name, c in clahe_table.items():
        assert not c["empty_bands"] or c["split"] == 1, name
    # the pitches of the LUT-loop shapes walk mis through every value on some entry of each shape
    for shape in ("1x1024", "1x1025", "16x1025", "16x2049"):
        assert any(clahe_table[n]["mis"] == list(range(16)) for n in clahe_table if n.startswith("lut_%s_p" % shape)), shape


def test_the_bound_shapes_stand_where_the_table_says(clahe_table):
    for ncols, nrows, tx, ty in ie.CLAHE_REFUSED:
        assert not ee.equalisable(ncols, nrows, tx, ty)
    a = ie.CLAHE_EDGES["large_a_4096x4112_2x2"]
    assert ee.equalisable(a.ncols, a.nrows, a.tiles_x, a.tiles_y)
    assert clahe_table["large_a_4096x4112_2x2"]["dxdy255"] == (1 << 32) - 65536 == 4294901760
    assert clahe_table["large_a_4096x4112_2x2"]["single_product"] >= 1 << 31
    assert clahe_table["large_c_4096x4200_1x1_constant"]["clip"][0][2] > 65000


def test_the_entries_stay_small():
    for table in (ie.CLAHE_EDGES, ie.REMAP_EDGES):
        for name, case in table.items():
            if name not in ie.LARGE_ENTRIES and name not in ie.REAL_ENTRIES:
                assert case.ncols * case.nrows <= 1100000, name
    assert len(ie.LARGE_ENTRIES) == 5 and all(ie.CLAHE_EDGES[n].ncols * ie.CLAHE_EDGES[n].nrows <= 4096 * 4200 for n in ie.LARGE_ENTRIES)
    assert all(n in ie.CLAHE_EDGES or n in ie.REMAP_EDGES for n in ie.REAL_ENTRIES)


# ----------------------------------------------------------------------------------------------------------------- remap classes
@pytest.fixture(scope="module")
def remap_table():
    out = {}
    for name, case in ie.REMAP_EDGES.items():
        _, (mx, my), _, stats = ie.remap_reference(name)
        out[name] = ie.remap_classes(case.ncols, case.nrows, mx, my, stats)
    return out


def _every_cut(ncols_list):
    """every (row & 3, lo of the first piece, hi of the last piece) the kernel can form on rows of those widths"""
    want = set()
    for ncols in ncols_list:
        for r in range(4):
            if any((y * ncols) & 3 == r for y in range(4)):
                last = (r + ncols) % 4
                want.add((r, r, last or 4))
    return want


def test_the_remap_table_reaches_every_class(remap_table):
    widths = list(range(1, 10)) + list(range(63, 70)) + list(range(127, 132))
    cuts = set()
    for n in remap_table:
        if n.startswith("cut_"):
            cuts |= set(remap_table[n]["cuts"])
    assert cuts == _every_cut(widths), cuts ^ _every_cut(widths)
    # lo is row & 3 and hi is (lo + ncols) % 4 (4 for 0); row & 3 takes every value under an odd width, 0 and 2 under ncols % 4 == 2 and
    # 0 alone under a multiple of 4: 4 + 4 + 2 + 1 pairs of (ragged start, ragged end)
    assert all(lo == r for r, lo, _ in cuts) and len({(lo, hi) for _, lo, hi in cuts}) == 11
    print("piece cuts (row & 3, lo, hi): %s" % sorted(cuts))
    classes = {
        "a row narrower than a piece, inside one": (lambda c: "one piece" in c["narrow"], ["cut_1x8_p1", "cut_2x8_p2", "cut_3x8_p3"]),
        "a row narrower than a piece, across two": (lambda c: "straddles two" in c["narrow"], ["cut_3x8_p3", "cut_3x8_p4"]),
        "remap_kernel<false>": (lambda c: c["kernel"] == "remap_kernel<false>", ["cut_1x8_p1", "lattice_1x169_noise", "extent_1x65535_wild"]),
        "remap_kernel<true>": (lambda c: c["kernel"] == "remap_kernel<true>", ["lattice_2x169_noise", "lattice_67x169_noise"]),
        "a grid of 1 x 1": (lambda c: c["grid"] == (1, 1), ["cut_1x8_p1", "cut_9x8_p9"]),
        "two workgroups across": (lambda c: c["grid"][0] == 2, ["cut_64x8_p64", "lattice_67x169_noise"]),
        "the widest grid, 1025 across": (lambda c: c["grid"][0] == 1025, ["extent_65535x1_wild"]),
        "a grid 4096 down": (lambda c: c["grid"][1] == 4096, ["extent_1x65535_wild", "extent_2x65535_wild"]),
        "all 169 clamp pairs": (lambda c: len(c["clamp_pairs"]) == 169, ["lattice_67x169_two_level", "lattice_67x169_noise"]),
        "all 169 clamp pairs on whole pieces": (lambda c: len(c["clamp_pairs_whole"]) == 169, ["lattice_67x169_two_level", "lattice_67x169_noise"]),
        "all 169 clamp pairs on ragged pieces": (lambda c: len(c["clamp_pairs_ragged"]) == 169, ["lattice_67x169_two_level", "lattice_67x169_noise"]),
        "an edge pair (x0 = ncols - 1, ncols >= 2)": (lambda c: c["edge_pair"], ["lattice_2x169_noise", "lattice_67x169_noise", "extent_2x65535_wild"]),
        "a weighted sum with low bits 0x8000": (lambda c: c["tie_8000"], ["tie_64x48_half_shift", "tie_640x480_both"]),
        "a weighted sum with low bits 0x7fff": (lambda c: c["tie_7fff"], ["tie_640x480_both"]),
    }
    for what, (holds, must) in classes.items():
        reached = [n for n, c in remap_table.items() if holds(c)]
        print("%s: %s" % (what, ", ".join(reached)))
        assert reached and set(must) <= set(reached), (what, must, reached)
    # the lattice on a frame 2 wide and 1 wide: the classes that fall together there are all reached
    for name, ncols in (("lattice_2x169_noise", 2), ("lattice_1x169_noise", 1)):
        distinct = len(set(ie.lattice_values(ncols)))
        assert len({p[0] for p in remap_table[name]["clamp_pairs"]}) == distinct and len({p[1] for p in remap_table[name]["clamp_pairs"]}) == 13


# ------------------------------------------------------------------------------------------------------------ wrong restatements
# the wrong step -> the entry whose expected bytes it changes
CLAHE_CAUGHT_BY = {
    "bins_mod_2_16": "count_256x256_constant_c0",
    "excess_mod_2_16": "count_256x257_constant_c1",
    "clip_product_mod_2_32": "count_256x257_constant_c1048576",
    "cap_without_max": "redist_16x17_cap_from_max",
    "remainder_to_first_bins": "redist_16x17_r15",
    "remainder_255_shifted": "redist_16x17_r255",
    "numerator_mod_2_32": "large_c_4096x4200_1x1_noise",
    "product_wrapped_int32": "large_a_4096x4112_2x2",
    "tie_downward": "apply_130x20_tx2",
    "edges_from_floor_width": "redist_67x45_3x2_two_bin",
}
REMAP_CAUGHT_BY = {
    "clamp_to_n": "lattice_67x169_noise",
    "no_min": "lattice_67x169_noise",
    "round_32767": "tie_64x48_half_shift",
    "fx_fy_exchanged": "tie_640x480_both",
    "clamp_after_shift": "lattice_67x169_noise",
}
# wrong steps that leave every byte as it is and show as a read outside the frame (the restatement raises IndexError): with the right
# clamp the weight of the pixel at x0 + 1 is 0 wherever x0 is the last column, so "no_min" changes addresses, not values; "clamp_to_n"
# makes x0 = ncols itself
READS_OUTSIDE = ("clamp_to_n", "no_min")


@pytest.mark.parametrize("wrong", [w for w in ie.CLAHE_WRONG if w != "centre_counted_with_gt"])
def test_a_wrong_clahe_rule_changes_a_named_entry(wrong):
    name = CLAHE_CAUGHT_BY[wrong]
    case = ie.CLAHE_EDGES[name]
    got = ie.clahe(ie.clahe_frame(case), case.tiles_x, case.tiles_y, case.clip_q8, wrong=wrong)
    differ = int((got != ie.clahe_reference(name)[0]).sum())
    print("%s: %d bytes of %s differ" % (wrong, differ, name))
    assert differ > 0


def test_a_pixel_on_a_centre_weighs_the_same_either_way():
    """`>` for `>=` at a pixel exactly on a centre is NO wrong rule: the pixel then counts as the far end of the interval before the
    centre, with w = D -- all weight on the same tile, and the division by D is exact.  So no entry can catch it; the table holds
    pixels on centres (tiles of odd width), and the two readings agree there byte for byte"""
    on_a_centre = 0
    for name, case in ie.CLAHE_EDGES.items():
        if name in ie.LARGE_ENTRIES or name in ie.REAL_ENTRIES:
            continue
        p = 2 * np.arange(case.ncols) + 1
        on_a_centre += int(np.isin(p, ie._centres(case.ncols, case.tiles_x)).sum())
        got = ie.clahe(ie.clahe_frame(case), case.tiles_x, case.tiles_y, case.clip_q8, wrong="centre_counted_with_gt")
        assert np.array_equal(got, ie.clahe_reference(name)[0]), name
    assert on_a_centre > 50


@pytest.mark.parametrize("wrong", ie.REMAP_WRONG)
def test_a_wrong_remap_rule_changes_a_named_entry(wrong):
    name = REMAP_CAUGHT_BY[wrong]
    frame, (mx, my), want, _ = ie.remap_reference(name)
    if wrong in READS_OUTSIDE:
        with pytest.raises(IndexError):
            ie.remap(frame, mx, my, wrong=wrong)
        return
    differ = int((ie.remap(frame, mx, my, wrong=wrong) != want).sum())
    print("%s: %d bytes of %s differ" % (wrong, differ, name))
    assert differ > 0


# ------------------------------------------------------------------------------------------------------------------------ draws
def test_the_draws_reach_the_trip_classes_and_the_clamp_pairs():
    trips, above = set(), 0
    for seed in ie.DRAW_SEEDS:
        frame, tx, ty, clip_q8, pitch = ie.clahe_draw(seed)
        nrows, ncols = frame.shape
        assert ncols <= 700 and nrows <= 500 and pitch >= ncols and ee.equalisable(ncols, nrows, tx, ty)
        w, h = int(np.diff(ie._edges(ncols, tx)).max()), int(np.diff(ie._edges(nrows, ty)).max())
        items = ((w + 30) >> 4) * h
        trips.add(min(3, -(-items // ie.LUT_THREADS)))
        above += items > ie.LUT_THREADS
    assert trips == {1, 2, 3} and above * 2 >= len(ie.DRAW_SEEDS), (trips, above)
    pairs = set()
    for seed in ie.DRAW_SEEDS:
        frame, (mx, my), pitch, name = ie.remap_draw(seed)
        nrows, ncols = frame.shape
        assert ncols <= 700 and nrows <= 500 and mx.dtype == np.int32 and mx.shape == frame.shape == my.shape
        if ncols >= 3 and nrows >= 3:                          # (below that, classes fall together)
            pairs |= ie.remap_classes(ncols, nrows, mx, my, dict(edge_pair=False, tie_8000=False, tie_7fff=False))["clamp_pairs"]
    print("clamp pairs in the draws: %d of 169" % len(pairs))
    assert len(pairs) >= 100
