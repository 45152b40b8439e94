"""(cpu) The sequences of tests/lean_state_expected.py -- the hand-written table and the seeded draws that tests/test_gpu_lean_readers.py
runs -- reach what they were written for: every operation kind on a lean slot and on a slot that holds both forms, every transition of
wants_lean, split batches in both outcomes, on-demand launches of 0, 1 and 2.  Conditions on the model's trace, not measurements.  And the
constants the model copies are the sources'."""
import os
import re

import lean_state_expected as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the readers whose launch has no lazy form under any list length: every one of them asks for the records
# (but the 9x9 launch, after which the taps change back and every slot is built full for that reason)
ASKERS = [k for k in L.READERS if k not in ("track_plain_batch", "track_plain_single", "shared_slot_batch", "track_w9")]


def _traces(lazy=1):
    out = {}
    for name, ops in [("fixed", L.fixed_table())] + [("seed %d" % s, L.seeded_sequence(s)) for s in L.SEEDS]:
        m = L.Model(lazy)
        out[name] = (ops, m.run(ops), m.builds)
    return out


TRACES = _traces()


def _asked(b):
    return {t for t in b["since"] if t.startswith("asked:")}


def test_every_kind_on_a_lean_slot_and_on_one_with_both_forms():
    ops, trace, _ = TRACES["fixed"]
    seen = {t["kind"] for name in TRACES for t in TRACES[name][1]}
    assert seen == set(L.KINDS), set(L.KINDS) ^ seen
    assert {t["kind"] for t in trace} == set(L.KINDS), "the fixed table alone reaches every kind"
    # (a window of 9 changes the smoothing taps -- the sigma is a factor times the window -- so under the adaptive rule no slot is lean
    # while it is set: option 2 alone brings a 9x9 launch to a lean slot, and the operation holds its own build and downloads)
    always = L.Model(2).run(ops)
    for kind in L.READERS:
        forms = [t["forms"] for t in (always if kind == "track_w9" else trace) if t["kind"] == kind]
        assert any(set(f) == {"lean"} for f in forms), "%s never runs on lean slots alone" % kind
        assert any(set(f) == {"both"} for f in forms), "%s never runs on slots that hold both forms" % kind
    assert {t["forms"][0] for t in trace if t["kind"] == "track_w9"} == {"full"}
    # ... directly after a lean build of new content, and directly after a download has made the records
    for kind in L.READERS:
        if kind == "track_w9":
            continue
        at = [i for i, t in enumerate(trace) if t["kind"] == kind]
        assert any(trace[i - 1]["kind"] == "build_all" and set(trace[i]["forms"]) == {"lean"} for i in at), kind
        assert any(trace[i - 1]["kind"] == "download" and set(trace[i]["forms"]) == {"both"} for i in at), kind
    swaps = [set(t["forms"][:2]) | set(t["forms"][2:]) for t in trace if t["kind"] == "swap_pairs"]
    assert any("lean" in s and len(s) > 1 for s in swaps), "no swap of a lean slot with one that holds records"
    # every plane of level 0, and level 1, which asks for nothing
    downloads = {(op[2], op[3]) for op in ops if op[0] == "download"}
    assert downloads >= {(0, 0), (1, 0), (2, 0), (0, 1)}
    assert all(t["demand"] == 0 for op, t in zip(ops, trace) if op[0] == "download" and op[3] == 1)
    grids = {op[2] for op in ops if op[0] == "select_grid"}
    assert grids == {1, 2}, "select_grid in both modes (2: KLT_REPLACING_SOME)"
    assert {op[2] for op in ops if op[0] == "track_light"} == {L.N_SHORT, L.N_LONG}, "the wave and the quad gain / bias kernels"


def test_every_transition_of_wants_lean():
    builds = [b for name in TRACES for b in TRACES[name][2]]
    fixed = TRACES["fixed"][2]
    for kind in ASKERS:                                    # true -> false through each kind of asker, alone
        assert any(b["before"] and not b["want"] and _asked(b) == {"asked:" + kind} for b in fixed), kind
    assert any(not b["before"] and b["want"] for b in fixed), "false -> true"
    assert any(b["before"] and b["want"] and b["lean"] for b in fixed), "stays lean"
    untouched = [b for b in builds if "lazy_read" in b["since"] and not _asked(b)]        # would be lean but for ...
    assert any(not b["want"] and b["resized"] and not b["retapped"] for b in untouched), "kept false by a changed frame size"
    assert any(not b["want"] and b["retapped"] and not b["resized"] for b in untouched), "kept false by changed taps"
    assert all(b["want"] for b in untouched if not b["resized"] and not b["retapped"])
    # a slot built alone between two batches: nothing read it since, so it is full in the second batch, the other 31 lean
    assert any(b["batch"] == L.NSLOTS and b["group"] == 1 and not b["want"] and not b["since"] for b in fixed)
    # the fallback of a launch that has a lazy form made the records and is not held against the slot; a launch without one is
    assert any("fallback" in b["since"] and not _asked(b) and b["want"] and b["lean"] for b in fixed)
    assert any(_asked(b) == {"asked:track_short"} and not b["want"] for b in fixed)
    # a wanted build below the bound is full and resets the slot: its next build is not wanted
    assert any(b["want"] and not b["lean"] for b in builds)


def test_split_batches_and_on_demand_launch_counts():
    trace = [t for name in TRACES for t in TRACES[name][1]]
    splits = [t["groups"] for t in trace if t["groups"] and len(t["groups"]) == 2]
    assert any(a[1] != b[1] for a, b in splits), "a split batch with a lean group"
    assert any(not a[1] and not b[1] for a, b in splits), "a split batch with both groups below the bound"
    assert any(a[1] and not b[1] for a, b in splits) and any(b[1] and not a[1] for a, b in splits), "the lean group first, and last"
    some = [t for t in trace if t["kind"] == "build_some"]
    assert any(t["lean"] for t in some) and any(not t["lean"] for t in some), "build_some above and below the bound"
    ops, fixed, _ = TRACES["fixed"]
    demand = {t["demand"] for t in fixed if t["kind"] in L.READERS}
    assert demand == {0, 1, 2}, demand          # (2: the two slots of a pair one after the other; no call of the ABI asks for two sizes at once)
    again = [i for i in range(1, len(ops)) if ops[i] == ops[i - 1] and ops[i][0] == "download" and ops[i][3] == 0]
    assert again and all(fixed[i]["demand"] == 0 for i in again) and any(fixed[i - 1]["demand"] == 1 for i in again), "a repeated ask"
    full = L.Model(0).run(ops)
    assert all(t["demand"] == 0 and not t["lean"] for t in full), "a context that never goes lean makes nothing on demand"
    always = L.Model(2).run(ops)
    assert all(t["lean"] == (t["groups"][-1][0] >= L.least_lean_batch()) for t in always if t["groups"])
    for stream, lean_form, form in ((2, 1, 2), (2, 0, 1), (1, 1, 2)):
        forms = {t["form"] for t in L.Model(1, stream, lean_form).run(ops) if t["groups"]}
        assert forms == {0, form}, (stream, lean_form, forms)


def test_sequence_sizes():
    assert len(L.SEEDS) == 8 and all(len(L.seeded_sequence(s)) >= len(L.PROLOGUE) + L.SEQUENCE_OPS for s in L.SEEDS)
    assert len({tuple(L.seeded_sequence(s)) for s in L.SEEDS}) == len(L.SEEDS)
    assert L.seeded_sequence(3) == L.seeded_sequence(3) and L.fixed_table() == L.fixed_table()
    assert len(L.fixed_table()) <= 320
    # the frame: lean at 32 frames on the wide strips, from least_lean_batch() frames on the narrow ones, never below
    assert L.NCOLS * L.NROWS * L.MAX_BATCH <= 34000000
    assert L.goes_lean(L.NCOLS, L.NROWS) and L.takes_geometry("wide", L.NCOLS, L.NROWS) and not L.takes_geometry("wide", L.NCOLS, L.NROWS, 31)
    low = L.least_lean_batch()
    assert 2 < low < L.MAX_BATCH and low == L.least_lean_batch(1) and not L.lean_launch(L.NCOLS, L.NROWS, low - 1, 2)
    assert L.NCOLS - 2 * L.BORDER >= 16 and L.NROWS - 2 * L.BORDER >= 16
    assert L.N_BATCH * L.NPAIRS == L.QUAD_MIN and L.N_LONG >= L.QUAD_MIN > L.N_SHORT and 3 * L.N_SHARED >= L.QUAD_MIN > 2 * L.N_SHARED


def test_constants_are_the_sources():
    def src(*parts):
        return open(os.path.join(REPO, *parts)).read()
    hdr = src("include", "klt_gpu.h")
    for name, value in (("TRACK_VARIANT", L.OPT_TRACK_VARIANT), ("BUILD_STREAM", L.OPT_BUILD_STREAM), ("TRACK_TREE_SUMS", L.OPT_TRACK_TREE_SUMS),
                        ("L0_STREAM", L.OPT_L0_STREAM), ("L0_LAZY_GRAD", L.OPT_L0_LAZY_GRAD), ("L0_LEAN_FORM", L.OPT_L0_LEAN_FORM)):
        assert int(re.search(r"#define\s+KLT_OPT_%s\s+(\d+)" % name, hdr).group(1)) == value, name
    assert int(re.search(r"#define\s+KLT_L0_LEAN_FORM_DEFAULT\s+(\d+)", hdr).group(1)) == 1
    plan = src("pyfeaturetrack_amd", "csrc", "l0_plan.h")
    assert re.search(r"L0S_MIN_WGS = (\d+), L0W_MIN_WGS = (\d+)", plan).groups() == (str(L.WORKGROUPS),) * 2
    assert int(re.search(r"constexpr int KLT_MAX_BATCH = (\d+);", plan).group(1)) == L.MAX_BATCH
    trk = src("pyfeaturetrack_amd", "csrc", "track_plan.h")
    assert int(re.search(r"constexpr long long TRACK_QUAD7_MIN = (\d+);", trk).group(1)) == L.QUAD_MIN
    assert re.search(r"const bool quad7 = q\.variant != 0 && wc\.wct == 7 && \(long long\)q\.n \* ny >= TRACK_QUAD7_MIN;", trk)
    # (over a sweep of launches: tests/test_track_plan_rule.py holds plan_track's lazy_capable against Model.lazy_capable)
    assert re.search(r"p\.lazy_capable = track_lazy_rule\(q\.fb, q\.guess, q\.light\) && quad7 && !q\.tree_sums && q\.n > 0 && ny > 0 && q\.grad7;", trk)
    frames = src("pyfeaturetrack_amd", "csrc", "api_frames.hip")
    assert "return c->l0_lazy_grad == 1 && s->lazy_read && !s->rec0_asked && s->built_nc == s->nc && s->built_nr == s->nr && s->built_cfg == c->cfg_gen;" in frames
    assert "B * (s0->nlev - 1) <= KLT_MAX_BATCH" in frames      # the merged gradient launch of a build's levels >= 1
    from helpers import make_tc
    tc = make_tc(levels=L.LEVELS, ss=L.SS)
    assert tc.borderx == tc.bordery == L.BORDER
