"""KLT_OPT_L0_LAZY_GRAD: every reader of level 0 and every state change of a slot, on a context that goes lean against one that never does.

Two contexts take the same options and the same calls in the same order: A under KLT_OPT_L0_LAZY_GRAD 0, B under 1 or 2.  After every
call of a sequence (tests/lean_state_expected.py: the hand-written table, eight seeded draws)
  * every list, quality table, affine state, selected list, prepared-key table and plane the call produced in B is byte-equal to A's;
  * after a build, B's klt_level0_lean and klt_level0_lean_form are the model's prediction and A's are false / 0;
  * the launches of family "gradients" the call sent out (klt_timing_read) are the model's prediction, in both contexts: a reader that
    forgot to ask for the records of a lean slot, or made records it already had, shows here if not in the bytes.
Since A is the code under test too, a sample of B's results on lean slots is held against the CPU oracle and the rules restated from it.

Frames: batches of 32 u8 frames of lean_state_expected.frame_shape() -- the smallest the production rule builds lean that has room for a
feature list inside the tracking border; a batch of fewer than least_lean_batch() frames has no lean form, so split batches fall on both
sides.  Every build uploads new content: the texture of synth.synth_base / shift_frame rolled by a phase of the step's own (the texture is
periodic: a roll by whole pixels is shift_frame's frame for that shift), pair i = slots (2 i, 2 i + 1) with the second frame moved by
(1.3, -0.8), a flat block at a fixed place.  Three levels, subsampling 4, max_residue 10.  No tolerances: every comparison is of bytes.

Lists (hand_list): tests/test_gpu_track_lazy.py's hand-placed list in small.  NaN positions sit in lost records and in the guess list, where
the suite already feeds them to the kernels; live records hold out-of-frame positions instead.  The affine check, whose kernel the suite
has only run on lists inside the frame, gets lists of live features inside the border and lost records.

The library has a switch that refuses a reader which would have to make records during a stream capture; the Python layer does not expose
it (tools/graph_frame_probe.py compiles a private copy), so that refusal is not tested here."""
import numpy as np
import pytest

import lean_state_expected as L
from helpers import make_tc, params_from_tc

REPLACING_SOME = 2
FLAT = (L.BORDER + 2, 1000, 12, 64)                  # x0, y0, width, height of the constant block in every frame
N_SELECT = 200
FB_L128, FB_LONG, FB_SHORT, FB_SHARED, FB_GUESS, FB_MOVED, FB_CLEAN, FB_CLEAN_LONG = 100, 130, 131, 132, 133, 135, 136, 137
OUT, BACK, QUAL = 200, 300, 400
SELECT_GRID = (8, 256, 2)                            # cells of 8 x 256 pixels, two features each
FB_MAX_ERROR = 0.5


def _tc(sigma=0.1, window=7, **attrs):
    """make_tc(levels=3, ss=4) with max_residue 10; the window of 9 keeps the border of 7 (or the frame's 17 columns inside it were none)
    and, to an ulp, the smoothing sigma (a factor times the window: 5 or 9 taps, or no launch were lean)"""
    if window != 7:
        attrs.update(borderx=L.BORDER, bordery=L.BORDER)
        sigma = sigma * 7 / window
    return make_tc(levels=L.LEVELS, ss=L.SS, window=window, max_residue=10.0, smooth_sigma_fact=sigma, **attrs)


# ------------------------------------------------------------------------------------------------------------------ frames and lists
@pytest.fixture(scope="module")
def frames0():
    """the 32 frames at phase (0, 0)"""
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(L.NCOLS, L.NROWS, 5)
    return [synth.shift_frame(base, 7.0 * (k // 2) + 1.3 * (k % 2), -3.0 * (k // 2) - 0.8 * (k % 2)) for k in range(L.NSLOTS)]


def content(frames0, k, step):
    """slot k's frame of step `step`: other pixels than any other step's"""
    f = np.roll(frames0[k], (29 * (step + 1) % L.NROWS, 17 * (step + 1) % L.NCOLS), axis=(0, 1))
    x0, y0, w, h = FLAT
    f[y0:y0 + h, x0:x0 + w] = 128
    return f


def hand_list(n, seed, clean=False, nan=True):
    """tests/test_gpu_track_lazy.py's _hand_list in small: live features inside the border; (not `clean`) on the border's edge and a
    step inside and outside it, at the frame's edges, out of the frame, on and around the flat block, a run of sub-pixel phases; lost
    records of every status, half of them with NaN positions"""
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    rng = np.random.default_rng([n, seed])
    W, H, B = L.NCOLS, L.NROWS, float(L.BORDER)
    fl = np.zeros(n, FEAT_DTYPE)
    fl["x"] = rng.uniform(B + 2, W - 1 - B - 2, n).astype(np.float32)
    fl["y"] = rng.uniform(B + 2, H - 1 - B - 2, n).astype(np.float32)
    if not clean:
        x0, y0, w, h = FLAT
        hand = [(x0 + 5.0 + 0.5 * i, y0 + 8.5 + 12 * i) for i in range(4)]                           # flat: small determinant
        for e in (0.0, 0.5, 1.31, -0.25):                                                             # distance from the border line
            hand += [(B + e, 300.25 + 40 * e), (W - 1 - B - e, 500.75), (B + 6.5, B + e), (B + 7.25, H - 1 - B - e)]
        hand += [(-5.0, 400.0), (128.0, -0.5), (W + 3.0, 400.0), (128.0, H + 0.25), (3.0, 600.5), (W - 4.0, 700.25), (125.5, 3.5),
                 (126.0, H - 4.5)]                                                                    # out of the frame, at its edges
        hand += [(x0 - 2.0 + 1.5 * i, y0 + 30.0) for i in range(8)] + [(x0 + 6.0, y0 + h - 4.0 + 1.5 * i) for i in range(6)]      # its edges
        hand += [(B + 4.0 + 0.125 * i, 1700.0 + 0.0625 * i) for i in range(16)]                       # a run of sub-pixel phases
        hand = hand[:n // 4]
        for i, (x, y) in enumerate(hand):
            fl["x"][4 * i], fl["y"][4 * i] = x, y
    lost = np.arange(1, n, 37)
    fl["val"][lost] = -1 - (np.arange(lost.size) % 5)
    fl["x"][lost[::2]] = np.nan if nan and not clean else -1.0
    fl["y"][lost[::2]] = np.nan if nan and not clean else -1.0
    return fl


def guess_list(fl, seed, nan=True):
    """the features' true positions plus noise; every seventh guess invalid, and (nan) NaN, inf and far-off positions among the rest"""
    rng = np.random.default_rng([len(fl), seed, 3])
    g = fl.copy()
    g["x"] = (fl["x"] + np.float32(1.3) + rng.normal(0, 1.0, len(fl))).astype(np.float32)
    g["y"] = (fl["y"] - np.float32(0.8) + rng.normal(0, 1.0, len(fl))).astype(np.float32)
    g["val"] = np.where(np.arange(len(fl)) % 7 == 3, -1, 0)
    if nan:
        g["x"][5::41] = np.nan
        g["y"][9::41] = np.inf
        g["x"][13::41] = 1e30
    return g


def moved(fl):
    """the list a quality launch reads as the tracked one: moved by the pair's shift, tracked"""
    m = fl.copy()
    m["x"] = (fl["x"] + np.float32(1.3)).astype(np.float32)
    m["y"] = (fl["y"] - np.float32(0.8)).astype(np.float32)
    return m


def all_lists(nan=True):
    lists = {FB_L128 + i: hand_list(L.N_BATCH, i, nan=nan) for i in range(L.NPAIRS)}
    lists.update({FB_LONG: hand_list(L.N_LONG, 1, nan=nan), FB_SHORT: hand_list(L.N_SHORT, 2, nan=nan), FB_SHARED: hand_list(L.N_SHARED, 3),
                  FB_CLEAN: hand_list(L.N_SHORT, 4, clean=True), FB_CLEAN_LONG: hand_list(L.N_LONG, 5, clean=True)})
    lists[FB_GUESS] = guess_list(lists[FB_SHORT], 6, nan)
    lists[FB_MOVED] = moved(lists[FB_SHORT])
    return lists


def select_mask():
    m = np.ones((L.NROWS, L.NCOLS), np.uint8)
    m[L.NROWS // 4:L.NROWS // 2, :] = 0
    m[::3, L.BORDER + 5] = 0
    return m


# ----------------------------------------------------------------------------------------------------------------------- the driver
class Rig:
    """the two contexts, their models and what the calls share"""

    def __init__(self, frames0, lazy, stream=2, lean_form=1, build_stream=0):
        from pyfeaturetrack_amd.backend import Context
        self.frames0, self.sigma, self.step = frames0, 0.1, 0
        self.lists, self.mask = all_lists(), select_mask()
        self.ctx, self.model = [], []
        for lz in (0, lazy):
            c = Context(0)
            self.ctx.append(c)
            c.configure(_tc())
            for opt, v in ((L.OPT_L0_STREAM, stream), (L.OPT_L0_LEAN_FORM, lean_form), (L.OPT_BUILD_STREAM, build_stream), (L.OPT_L0_LAZY_GRAD, lz)):
                c.set_option(opt, v)
            for fb, fl in self.lists.items():
                c.featbuf_upload(fb, fl)
            self.model.append(L.Model(lz, stream, lean_form))

    def close(self):
        for c in self.ctx:
            c.set_option(L.OPT_TRACK_VARIANT, 4)         # (process-wide)
            c.close()

    def call(self, c, op):
        """one operation on one context: ([bytes the call produced], (klt_level0_lean, klt_level0_lean_form) after a build or None)"""
        from pyfeaturetrack_amd.params import affine_params_from_tc
        kind, ids = op[0], L.slots_of(op)
        lists, n_of = self.lists, {FB_LONG: L.N_LONG, FB_SHORT: L.N_SHORT, FB_CLEAN: L.N_SHORT, FB_CLEAN_LONG: L.N_LONG}

        def records(fbs, n):
            c.sync()
            return [c.featbuf_download(fb, n).tobytes() for fb in fbs]

        def build(frames):
            for k, f in zip(ids, frames):
                c.upload(k, f)
            c.build_pyramids_batch(ids, sync=True)
            return [], (c.level0_lean(), c.level0_lean_form())

        if kind in ("build_all", "build_some", "build_one"):
            return build([content(self.frames0, k, self.step) for k in ids])
        if kind == "build_other_size":
            build([content(self.frames0, ids[0], self.step)[:-1]])
            return build([content(self.frames0, ids[0], self.step)])
        if kind in ("track_plain_batch", "track_variant0"):
            if kind == "track_variant0":
                c.set_option(L.OPT_TRACK_VARIANT, 0)
            try:
                c.track_batch_async([(2 * i, 2 * i + 1, FB_L128 + i, OUT + i) for i in range(L.NPAIRS)], L.N_BATCH)
                return records([OUT + i for i in range(L.NPAIRS)], L.N_BATCH), None
            finally:
                c.set_option(L.OPT_TRACK_VARIANT, 4)
        if kind == "shared_slot_batch":
            c.track_batch_async([(0, 1, FB_SHARED, OUT), (1, 2, FB_SHARED, OUT + 1), (2, 3, FB_SHARED, OUT + 2)], L.N_SHARED)
            return records([OUT, OUT + 1, OUT + 2], L.N_SHARED), None
        s1, s2 = (ids + ids + [None, None])[:2]
        if kind in ("track_plain_single", "track_short", "track_tree_sums", "track_w9", "track_light"):
            fb = FB_SHORT if kind == "track_short" or (kind == "track_light" and op[2] == L.N_SHORT) else FB_LONG
            extra, report = [], None
            try:
                if kind == "track_tree_sums":
                    c.set_option(L.OPT_TRACK_TREE_SUMS, 1)
                if kind == "track_w9":                       # (other taps: every slot is built anew under them)
                    c.configure(_tc(self.sigma, 9))
                    for k in range(L.NSLOTS):
                        c.upload(k, content(self.frames0, k, self.step))
                    c.build_pyramids_batch(list(range(L.NSLOTS)), sync=True)
                    report = (c.level0_lean(), c.level0_lean_form())
                    if op[2]:
                        extra = [c.download_level(k, 2, 0).tobytes() for k in (s1, s2)]
                if kind == "track_light":
                    c.set_light_params(mode=1)
                c.track_async(s1, s2, fb, OUT, n_of[fb])
                out = records([OUT], n_of[fb])
                if kind == "track_light":
                    extra = [bytes([c.track_light_path()])]
                    assert extra[0][0] == (1 if op[2] == L.N_SHORT else 2), "the gain / bias kernel the operation was written for"
                return out + extra, report
            finally:
                c.set_option(L.OPT_TRACK_TREE_SUMS, 0)
                c.set_light_params(mode=0)
                if kind == "track_w9":
                    c.configure(_tc(self.sigma, 7))
        if kind == "track_fb":
            c.set_fb_params(max_error=FB_MAX_ERROR)
            if not op[2]:
                c.track_fb_async(s1, s2, FB_SHORT, OUT, L.N_SHORT, fb_back=BACK)
                return records([OUT, BACK], L.N_SHORT), None
            c.track_fb_batch_async([(ids[0], ids[1], FB_SHORT, OUT, BACK), (ids[2], ids[3], FB_SHORT, OUT + 1, BACK + 1)], L.N_SHORT)
            return records([OUT, OUT + 1, BACK, BACK + 1], L.N_SHORT), None
        if kind == "track_guess":
            if not op[2]:
                c.track_guess_async(s1, s2, FB_SHORT, FB_GUESS, OUT, L.N_SHORT)
                return records([OUT], L.N_SHORT), None
            c.track_guess_batch_async([(ids[0], ids[1], FB_SHORT, FB_GUESS, OUT), (ids[2], ids[3], FB_SHORT, -1, OUT + 1)], L.N_SHORT)
            return records([OUT, OUT + 1], L.N_SHORT), None
        if kind == "track_fb_guess":
            c.set_fb_params(max_error=FB_MAX_ERROR)
            c.track_fb_guess_async(s1, s2, FB_SHORT, FB_GUESS, OUT, L.N_SHORT, fb_back=BACK)
            return records([OUT, BACK], L.N_SHORT), None
        if kind == "track_affine":
            fb = FB_CLEAN if op[2] == L.N_SHORT else FB_CLEAN_LONG
            try:
                c.set_affine_params(affine_params_from_tc(_tc(self.sigma, affineConsistencyCheck=2)))
                c.affine_alloc(0, op[2])
                c.track_affine_async(s1, s2, fb, OUT, op[2], 0)
                return records([OUT], op[2]) + [c.affine_download(0, op[2]).tobytes()], None
            finally:
                c.set_affine_params(affine_params_from_tc(_tc(self.sigma)))
        if kind == "quality_single":
            c.track_quality_async(s1, s2, FB_SHORT, FB_MOVED, QUAL, L.N_SHORT)
            return records([QUAL], L.N_SHORT), None
        if kind == "quality_batch":
            c.track_quality_batch_async([(ids[2 * j], ids[2 * j + 1], FB_SHORT, FB_MOVED, QUAL + j) for j in range(op[2])], L.N_SHORT)
            return records([QUAL + j for j in range(op[2])], L.N_SHORT), None
        if kind in ("select", "select_masked", "select_grid", "select_prepared"):
            out = []
            try:
                if kind == "select_masked":
                    c.set_select_mask(self.mask)
                if kind == "select_grid":
                    c.set_select_grid(SELECT_GRID)
                if kind == "select_prepared":
                    c.select_prepare(s1)
                    c.sync()
                    out.append(c.prepared_keys(s1).tobytes())
                if kind == "select_prepared" or (kind == "select_grid" and op[2] == REPLACING_SOME):
                    fl, placed = c.select(s1, N_SELECT, mode=REPLACING_SOME, fl=lists[FB_CLEAN][:N_SELECT], use_pyramid=True)
                else:
                    fl, placed = c.select(s1, N_SELECT, use_pyramid=True)
                return out + [fl.tobytes(), bytes([placed % 256])], None
            finally:
                c.set_select_mask(None)
                c.set_select_grid(None)
        if kind == "download":
            return [c.download_level(s1, op[2], op[3]).tobytes()], None
        if kind == "swap_pairs":
            for a, b in zip(L.pair_slots(op[1]), L.pair_slots(op[2])):
                c.swap_slots(a, b)
            return [], None
        if kind == "retap":
            c.configure(_tc(0.2 if self.sigma == 0.1 else 0.1))
            return [], None
        raise KeyError(kind)

    def run(self, ops):
        for self.step, op in enumerate(ops):
            got = []
            for c, m in zip(self.ctx, self.model):
                want = m.apply(op)
                c.timing_enable(True)
                try:
                    out, report = self.call(c, op)
                    c.sync()
                    grads = {t["name"]: t["launches"] for t in c.timing_read()}.get("gradients", 0)
                finally:
                    c.timing_enable(False)
                got.append((out, report, grads, want))
            if op[0] == "retap":
                self.sigma = 0.2 if self.sigma == 0.1 else 0.1
            (oa, ra, ga, wa), (ob, rb, gb, wb) = got
            what = "step %d, %r" % (self.step, op)
            print(what, "A:", ra, ga, "B:", rb, gb, "model:", wa["grads"], wb["grads"], wb["lean"], wb["form"], wb["forms"])
            assert len(oa) == len(ob)
            for i, (x, y) in enumerate(zip(oa, ob)):
                assert x == y, "%s: result %d of the lean context differs from the full context's" % (what, i)
            if wb["groups"] is not None:
                assert ra == (False, 0), "%s: the context that never goes lean reports %r" % (what, ra)
                assert rb == (wb["lean"], wb["form"]), "%s: klt_level0_lean / _form say %r, the rule %r" % (what, rb, (wb["lean"], wb["form"]))
            assert ga == wa["grads"], "%s: %d gradient launches in the full context, the rule says %d" % (what, ga, wa["grads"])
            assert gb == wb["grads"], "%s: %d gradient launches in the lean context, the rule says %d (%d of them on demand)" % (
                what, gb, wb["grads"], wb["demand"])


VARIANTS = {"adaptive": dict(lazy=1), "always": dict(lazy=2), "always-banded": dict(lazy=2, lean_form=0), "adaptive-narrow": dict(lazy=1, stream=1),
            "adaptive-build-stream": dict(lazy=1, build_stream=1)}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fixed_sequence(frames0, variant):
    """the hand-written table: every reader kind directly after a lean build of new content and directly after a download has made the
    records, then swaps, partial builds on both sides of the bound, a slot built alone, a changed size, changed taps, split batches"""
    rig = Rig(frames0, **VARIANTS[variant])
    try:
        rig.run(L.fixed_table())
    finally:
        rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", [1, 2])
@pytest.mark.parametrize("seed", L.SEEDS)
def test_seeded_sequence(frames0, seed, lazy):
    rig = Rig(frames0, lazy)
    try:
        rig.run(L.seeded_sequence(seed))
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ a sample, by the oracle
@pytest.fixture(scope="module")
def sample(frames0):
    """one context under option 2, the frames of one step, and the oracle's pyramids of slots 0, 1 and 31 (made when first asked for)"""
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    c.configure(_tc())
    c.set_option(L.OPT_L0_LAZY_GRAD, 2)
    lists = all_lists(nan=False)
    for fb, fl in lists.items():
        c.featbuf_upload(fb, fl)
    fr = [content(frames0, k, 1000) for k in range(L.NSLOTS)]
    p = params_from_tc(_tc())
    pyr = {}

    def pyramid(k):
        if k not in pyr:
            ko.set_threads(8)
            try:
                pyr[k] = ko.Pyramids(p, fr[k].astype(np.float32))
            finally:
                ko.set_threads(1)
        return pyr[k]

    def lean_build():
        for k, f in enumerate(fr):
            c.upload(k, f)
        c.build_pyramids_batch(list(range(L.NSLOTS)), sync=True)
        assert c.level0_lean() and c.level0_lean_form() == 2

    yield dict(ctx=c, lists=lists, frames=fr, p=p, pyramid=pyramid, lean_build=lean_build, ko=ko)
    c.close()


def _same(got, want, what):
    for k in ("val", "x", "y"):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), "%s: %s differs from the rule's at %r" % (
            what, k, np.flatnonzero(got[k] != np.asarray(want[k]).astype(got[k].dtype))[:8])


def _oracle_tracker(s):
    ko, p = s["ko"], s["p"]

    def track(fl, a, b):
        out = fl.copy()
        ko.track_features(p, s["pyramid"](a - 1), s["pyramid"](b - 1), out)
        return out
    return track


@pytest.mark.gpu
@pytest.mark.parametrize("reader", ["plain", "fb", "guess", "light", "quality", "select", "planes"])
def test_sample_against_the_oracle(sample, reader):
    """pair (0, 1) directly after a lean build: each reader's result is the CPU oracle's, or the rule restated from it, exactly"""
    from fb_expected import fb_compose
    from guess_expected import guess_compose
    from light_expected import light_track
    from quality_expected import quality_expected
    from select_mask_expected import select_expected
    s = sample
    c, ko, p, lists = s["ctx"], s["ko"], s["p"], s["lists"]
    s["lean_build"]()
    fin = lists[FB_SHORT]
    if reader == "plain":
        c.track_async(0, 1, FB_LONG, OUT, L.N_LONG)
        c.sync()
        got = c.featbuf_download(OUT, L.N_LONG)
        want = _oracle_tracker(s)(lists[FB_LONG], 1, 2)
        _same(got, want, "plain tracker")
        assert (got["val"] == 0).sum() > L.N_LONG // 2
    elif reader == "fb":
        c.set_fb_params(max_error=FB_MAX_ERROR)
        c.track_fb_async(0, 1, FB_SHORT, OUT, L.N_SHORT, fb_back=BACK)
        c.sync()
        want, _, wback = fb_compose(_oracle_tracker(s), fin, FB_MAX_ERROR)
        _same(c.featbuf_download(OUT, L.N_SHORT), want, "forward-backward")
        _same(c.featbuf_download(BACK, L.N_SHORT), wback, "forward-backward, backward records")
    elif reader == "guess":
        c.track_guess_async(0, 1, FB_SHORT, FB_GUESS, OUT, L.N_SHORT)
        c.sync()
        _same(c.featbuf_download(OUT, L.N_SHORT), guess_compose(ko, p, s["pyramid"](0), s["pyramid"](1), fin, lists[FB_GUESS]), "motion prior")
    elif reader == "light":
        try:
            c.set_light_params(mode=1)
            c.track_async(0, 1, FB_SHORT, OUT, L.N_SHORT)
            c.sync()
        finally:
            c.set_light_params(mode=0)
        _same(c.featbuf_download(OUT, L.N_SHORT), light_track(p, s["pyramid"](0), s["pyramid"](1), fin), "gain / bias tracker")
    elif reader == "quality":
        c.track_quality_async(0, 1, FB_SHORT, FB_MOVED, QUAL, L.N_SHORT)
        c.sync()
        want = quality_expected(ko, s["pyramid"](0), s["pyramid"](1), fin, lists[FB_MOVED], 7)
        got = c.quality_download(QUAL, L.N_SHORT)
        assert got.tobytes() == want.tobytes(), "quality records differ from the rule's at %r" % np.flatnonzero(got != want)[:8]
        assert (got["val"] == 1).sum() > L.N_SHORT // 2
    elif reader == "select":
        got, placed = c.select(0, N_SELECT, use_pyramid=True)
        want = select_expected(p, s["frames"][0], N_SELECT)
        _same(got, want, "selection")
        assert placed == int((want["val"] >= 0).sum()) > 0
    else:
        for k in (0, L.NSLOTS - 1):
            for plane, name in ((1, "gx"), (2, "gy")):
                got = c.download_level(k, plane, 0)
                assert got.tobytes() == np.ascontiguousarray(s["pyramid"](k).level(name, 0)).tobytes(), "slot %d, %s of level 0" % (k, name)
