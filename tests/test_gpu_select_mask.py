"""Selection mask (klt_set_select_mask / klt_set_select_mask_device, tc.selectionMask) on the GPU: every record equals the list composed
from the pinned oracle's pieces (tests/select_mask_expected.py) bit for bit -- x, y and val."""
import os

import numpy as np
import pytest

from conftest import read_pgm
from helpers import _api_modules, make_tc, params_from_tc
from select_mask_expected import (GOLDEN, REPLACING_SOME, SELECTING_ALL, drop_every_third, frame, inside_rect, rect_mask, rect_of,
                                  same_records, select_expected, window_mask)

pytestmark = pytest.mark.gpu
KLT_OPT_TOPK_PREFILTER, KLT_OPT_SELECT_PARALLEL_NMS, KLT_OPT_FAIL_ALLOC_AFTER = 5, 8, 19
MODES = [SELECTING_ALL, REPLACING_SOME]

_frames, _expected = {}, {}


def frame_of(ncols, nrows):
    """the frames every test shares: tests/golden/img0.pgm at 320 x 240, a synthetic texture otherwise"""
    if (ncols, nrows) not in _frames:
        _frames[ncols, nrows] = read_pgm(os.path.join(GOLDEN, "img0.pgm")) if (ncols, nrows) == (320, 240) else frame(ncols, nrows)
    return _frames[ncols, nrows]


def count_of(ncols):
    return 500 if ncols == 720 else (30 if ncols == 160 else 100)


def masks_of(ncols, nrows):
    return {"none": None, "rect": rect_mask(ncols, nrows), "window": window_mask(ncols, nrows),
            "zeros": np.zeros((nrows, ncols), np.uint8), "ones": np.ones((nrows, ncols), np.uint8)}


def expected(ncols, nrows, mode, mask_name, **tc_attrs):
    """(list the selection starts from, expected records), computed once per case and never modified"""
    key = (ncols, nrows, mode, mask_name, tuple(sorted(tc_attrs.items())))
    if key not in _expected:
        p = params_from_tc(make_tc(**tc_attrs))
        img, n = frame_of(ncols, nrows).astype(np.float32), count_of(ncols)
        start = None
        if mode == REPLACING_SOME:                       # every third feature of the unmasked selection lost
            start = drop_every_third(expected(ncols, nrows, SELECTING_ALL, "none", **tc_attrs)[1])
        want = select_expected(p, img, n, mode, start, masks_of(ncols, nrows)[mask_name])
        for a in (start, want):
            if a is not None:
                a.setflags(write=False)
        _expected[key] = (start, want)
    return _expected[key]


class Ctx:
    """a context with the shared frame of one size in slot 0, its pyramids built"""

    def __init__(self, ncols, nrows, options=(), **tc_attrs):
        from pyfeaturetrack_amd.backend import Context
        self.size = (ncols, nrows)
        self.c = Context(0)
        try:
            self.c.configure(make_tc(**tc_attrs))
            for opt, value in options:
                self.c.set_option(opt, value)
            self.c.upload(0, frame_of(ncols, nrows))
            self.c.build_pyramids(0, sync=True)
        except Exception:
            self.c.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.close()

    def select(self, mode, start=None, use_pyramid=True):
        return self.c.select(0, count_of(self.size[0]), mode, start, use_pyramid)[0]


def check(got, want, what):
    assert np.array_equal(got["val"], want["val"]), "%s: status / value words" % (what,)
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["y"], want["y"]), "%s: positions" % (what,)


# ---- 1: basic, both modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(320, 240), (322, 241)], ids=lambda s: "%dx%d" % s)
def test_rectangle_mask_both_modes(size):
    """322 x 241: ncols % 4 != 0 (the barrier-coupled table kernels) and ncols * nrows % 16 != 0 (the stamp kernel's tail)"""
    ncols, nrows = size
    rect = rect_of(ncols, nrows)
    with Ctx(ncols, nrows) as g:
        g.c.set_select_mask(rect_mask(ncols, nrows))
        for use_pyramid in (False, True):
            got = g.select(SELECTING_ALL, use_pyramid=use_pyramid)
            check(got, expected(ncols, nrows, SELECTING_ALL, "rect")[1], ("all", use_pyramid))
            assert not inside_rect(got, rect).any()
            start, want = expected(ncols, nrows, REPLACING_SOME, "rect")
            live = start["val"] >= 0
            assert inside_rect(start, rect).any(), "no live feature inside the masked rectangle: the case shows nothing"
            got = g.select(REPLACING_SOME, start, use_pyramid=use_pyramid)
            check(got, want, ("replace", use_pyramid))
            assert np.array_equal(got[live], start[live]), "live features (those inside the masked rectangle too) come back unchanged"
            assert not inside_rect(got[~live], rect).any() and (got["val"][~live] >= 0).all()
        # the eigenvalue map of a masked selection reads 0 at masked candidates (as in the live features' squares)
        p = params_from_tc(make_tc())
        bx, by = int(max(p.borderx, p.window_width / 2.0)), int(max(p.bordery, p.window_height / 2.0))
        g.select(SELECTING_ALL, use_pyramid=False)
        val = g.c.select_intermediate(3)
        at = rect_mask(ncols, nrows)[by:, bx:][:val.shape[0], :val.shape[1]]
        assert (val[at == 0] == 0).all() and (val[at != 0] > 0).any()


# ---- 2, 3: pitch > ncols, device mask ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["all", "replace"])
def test_padded_host_mask_and_device_mask_equal_the_compact_host_mask(mode):
    ncols, nrows = 322, 241
    start, want = expected(ncols, nrows, mode, "rect")
    mask = rect_mask(ncols, nrows)
    with Ctx(ncols, nrows) as g:
        wide = np.zeros((nrows, ncols + 13), np.uint8)          # what lies behind a row's end must not matter: zeros would mask
        wide[:, :ncols] = mask
        view = wide[:, :ncols]
        assert view.strides == (ncols + 13, 1)
        g.c.set_select_mask(view)
        check(g.select(mode, start), want, "pitch = ncols + 13")
        g.c.set_select_mask(None)
        dev = g.c.device_alloc(ncols * nrows)                    # exactly the mask: nothing behind byte ncols * nrows - 1 is the caller's
        g.c.device_write(dev, mask)
        g.c.set_select_mask_device(dev, ncols, nrows)
        check(g.select(mode, start), want, "device mask")
        # read in place: other contents at the same address, no call in between
        g.c.device_write(dev, window_mask(ncols, nrows))
        check(g.select(mode, start), expected(ncols, nrows, mode, "window")[1], "device mask rewritten in place")
        g.c.set_select_mask_device(None, 0, 0)
        check(g.select(mode, start), expected(ncols, nrows, mode, "none")[1], "device mask removed")
        from pyfeaturetrack_amd.backend import KltBackendError
        with pytest.raises(KltBackendError, match="error -1.*multiple of 16"):
            g.c.set_select_mask_device(dev + 3, ncols, nrows)
        g.c.device_free(dev)


# ---- 4: 720 x 480, the candidate prefilter and its fallback -----------------------------------------------------------------------
@pytest.mark.parametrize("options", [(), ((KLT_OPT_TOPK_PREFILTER, 0),), ((KLT_OPT_SELECT_PARALLEL_NMS, 0),)],
                         ids=["default", "no-prefilter", "serial-walk"])
def test_720x480_prefilter_fallback_and_serial_walk(options):
    """more than 262144 candidates: the prefilter is active by default.  Under the 64 x 64 window mask the candidates run out, so the
    selection falls back to every candidate and must still give the expected short list"""
    ncols, nrows = 720, 480
    with Ctx(ncols, nrows, options) as g:
        for name in ("rect", "window"):
            g.c.set_select_mask(masks_of(ncols, nrows)[name])
            for mode in MODES:
                start, want = expected(ncols, nrows, mode, name)
                check(g.select(mode, start), want, (name, mode))
            if name == "window":
                want = expected(ncols, nrows, SELECTING_ALL, name)[1]
                assert 0 < (want["val"] >= 0).sum() < count_of(ncols)


# ---- 5: prepared scores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect", "window"])
def test_prepared_scores_at_720x480(name):
    from pyfeaturetrack_amd.backend import KltBackendError
    ncols, nrows = 720, 480
    n = count_of(ncols)
    start, want = expected(ncols, nrows, REPLACING_SOME, name)
    with Ctx(ncols, nrows) as g:
        g.c.set_select_mask(masks_of(ncols, nrows)[name])
        plain = g.select(REPLACING_SOME, start)
        g.c.select_intermediate(3)                               # (scored by the selection itself: there is an eigenvalue map)
        g.c.select_prepare(0)
        prepared = g.select(REPLACING_SOME, start)
        with pytest.raises(KltBackendError, match="prepared scores"):
            g.c.select_intermediate(3)                           # the prepared scores WERE used
        check(prepared, plain, "with and without the preparation")
        check(prepared, want, "prepared scores against the oracle")
        # the two halves, the mask's contents changed between them: it was read by the first half (the window mask's fallback to every
        # candidate runs inside the second half and must reuse the stamped seed map)
        g.c.set_select_mask(None)
        dev = g.c.device_alloc(ncols * nrows)
        g.c.device_write(dev, masks_of(ncols, nrows)[name])
        g.c.set_select_mask_device(dev, ncols, nrows)
        g.c.select_prepare(0)
        g.c.featbuf_upload(7, start)
        g.c.select_begin(0, REPLACING_SOME, True, 7, n)
        g.c.device_write(dev, np.zeros((nrows, ncols), np.uint8))
        g.c.select_finish()
        check(g.c.featbuf_download(7, n), want, "mask contents changed between the two halves")


# ---- 6: mindist = 0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["all", "replace"])
def test_no_minimum_distance(mode):
    """no live squares to mark (a replacement passed no seed map at all before there were masks): the mask alone fills the map"""
    ncols, nrows = 322, 241
    start, want = expected(ncols, nrows, mode, "rect", mindist=0)
    with Ctx(ncols, nrows, mindist=0) as g:
        g.c.set_select_mask(rect_mask(ncols, nrows))
        got = g.select(mode, start)
        check(got, want, "mindist 0")
        placed = got if start is None else got[start["val"] < 0]
        assert not inside_rect(placed, rect_of(ncols, nrows)).any()


# ---- 7: degenerate masks ----------------------------------------------------------------------------------------------------------
def test_degenerate_masks():
    ncols, nrows = 322, 241
    with Ctx(ncols, nrows) as g:
        unmasked = {mode: g.select(mode, expected(ncols, nrows, mode, "none")[0]) for mode in MODES}
        for mode in MODES:
            check(unmasked[mode], expected(ncols, nrows, mode, "none")[1], "no mask")
        g.c.set_select_mask(np.zeros((nrows, ncols), np.uint8))
        got = g.select(SELECTING_ALL)
        assert (got["x"] == -1).all() and (got["y"] == -1).all() and (got["val"] == -1).all()
        check(got, expected(ncols, nrows, SELECTING_ALL, "zeros")[1], "all-zero mask")
        start = expected(ncols, nrows, REPLACING_SOME, "zeros")[0]
        got = g.select(REPLACING_SOME, start)
        check(got, start, "all-zero mask: nothing is replaced")
        g.c.set_select_mask(np.ones((nrows, ncols), np.uint8))
        for mode in MODES:
            check(g.select(mode, expected(ncols, nrows, mode, "none")[0]), unmasked[mode], "all-ones mask")
        g.c.set_select_mask(rect_mask(ncols, nrows))
        assert not same_records(g.select(SELECTING_ALL), unmasked[SELECTING_ALL])
        g.c.set_select_mask(None)
        for mode in MODES:
            check(g.select(mode, expected(ncols, nrows, mode, "none")[0]), unmasked[mode], "mask removed")


# ---- 8: stamp wrap ----------------------------------------------------------------------------------------------------------------
def test_260_selections_across_the_stamp_wrap():
    """the seed map's stamps run 1 .. 255 and the map is cleared at the wrap: two masks alternate (255 is odd, so a stamp comes round
    under the OTHER mask), and a stale stamp -- or a map not cleared -- would block pixels the current mask allows"""
    ncols, nrows = 160, 120
    names = ("rect", "window")
    assert not same_records(expected(ncols, nrows, SELECTING_ALL, "rect")[1], expected(ncols, nrows, SELECTING_ALL, "window")[1])
    with Ctx(ncols, nrows) as g:
        for i in range(1, 261):
            name = names[i % 2]
            mode = REPLACING_SOME if i % 5 == 0 else SELECTING_ALL
            g.c.set_select_mask(masks_of(ncols, nrows)[name])
            start, want = expected(ncols, nrows, mode, name)
            check(g.select(mode, start), want, "selection %d (%s, mode %d)" % (i, name, mode))


# ---- 9: errors --------------------------------------------------------------------------------------------------------------------
def test_mask_of_another_size_and_mask_set_while_pending():
    from pyfeaturetrack_amd.backend import KltBackendError
    ncols, nrows = 322, 241
    n = count_of(ncols)
    with Ctx(ncols, nrows) as g:
        g.c.set_select_mask(rect_mask(320, 240))
        with pytest.raises(KltBackendError, match=r"error -1.*320 x 240.*322 x 241"):
            g.select(SELECTING_ALL)
        g.c.set_select_mask(rect_mask(ncols, nrows))
        check(g.select(SELECTING_ALL), expected(ncols, nrows, SELECTING_ALL, "rect")[1], "after the refused call")
        dev = g.c.device_alloc(ncols * nrows)
        g.c.select_begin(0, SELECTING_ALL, True, 7, n)
        for call in (lambda: g.c.set_select_mask(window_mask(ncols, nrows)), lambda: g.c.set_select_mask(None),
                     lambda: g.c.set_select_mask_device(dev, ncols, nrows), lambda: g.c.set_select_mask_device(None, 0, 0)):
            with pytest.raises(KltBackendError, match="error -3.*pending"):
                call()
        g.c.select_finish()
        check(g.c.featbuf_download(7, n), expected(ncols, nrows, SELECTING_ALL, "rect")[1], "the pending selection kept its mask")
        with pytest.raises(KltBackendError, match="error -1"):
            g.c._check(g.c._lib.klt_set_select_mask(g.c._h, rect_mask(ncols, nrows).ctypes.data, ncols, nrows, ncols - 1))


def test_refused_allocations_of_a_first_masked_selection():
    """KLT_OPT_FAIL_ALLOC_AFTER walked over every allocation of klt_set_select_mask + the first masked selection of a context (the mask
    plane, the feature buffer, the selection's scratch, the seed map, ...): KLT_ERR_NOMEM each time, the same call again succeeds"""
    from pyfeaturetrack_amd.backend import KltOutOfMemory
    ncols, nrows = 322, 241
    start, want = expected(ncols, nrows, REPLACING_SOME, "rect")
    refused = []
    for k in range(64):
        with Ctx(ncols, nrows) as g:
            fired = []

            def attempt(what, fn):
                try:
                    return fn()
                except KltOutOfMemory as e:
                    assert "bytes asked for" in str(e) and "error -4" in str(e), str(e)
                    fired.append(what)
                    return fn()                                    # the hook has fired (it disarms itself): the same call again
            g.c.set_option(KLT_OPT_FAIL_ALLOC_AFTER, k)
            try:
                attempt("mask", lambda: g.c.set_select_mask(rect_mask(ncols, nrows)))
                got = attempt("select", lambda: g.select(REPLACING_SOME, start, use_pyramid=False))
            finally:
                g.c.set_option(KLT_OPT_FAIL_ALLOC_AFTER, -1)
            check(got, want, "allocation %d refused" % k)
            if not fired:
                break
            assert len(fired) == 1
            refused.append(fired[0])
    else:
        pytest.fail("the sequence never ran out of allocation sites")
    # the mask plane, then the feature buffer, four scratch planes, keys, convolution scratch, seed map, slot list, the passes' buffers ...
    assert refused[0] == "mask" and refused.count("select") >= 10, refused


# ---- 10: Python API ---------------------------------------------------------------------------------------------------------------
def _recs(fl):
    out = np.zeros(len(fl), [("x", np.float32), ("y", np.float32), ("val", np.int32)])
    out["x"], out["y"], out["val"] = [f.x for f in fl], [f.y for f in fl], [f.val for f in fl]
    return out


def test_python_api_mask_kinds_and_in_place_change():
    from PIL import Image
    sgf, _ = _api_modules()
    ncols, nrows = 320, 240
    img, n = frame_of(ncols, nrows), count_of(ncols)
    want = expected(ncols, nrows, SELECTING_ALL, "rect")[1]
    tc = make_tc()
    mask = rect_mask(ncols, nrows)
    for given in (mask.astype(bool), Image.fromarray(mask * 255), mask.astype(np.int32) * 1000):
        tc.selectionMask = given
        check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), want, type(given).__name__)
    tc.selectionMask = mask                                      # the very array: changed in place below
    check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), want, "uint8 array")
    mask[:] = window_mask(ncols, nrows)
    check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), expected(ncols, nrows, SELECTING_ALL, "window")[1], "changed in place")
    mask[:] = rect_mask(ncols, nrows)
    fl = sgf.KLTSelectGoodFeatures(tc, img, n)
    start, want_rep = expected(ncols, nrows, REPLACING_SOME, "rect")
    unmasked = expected(ncols, nrows, SELECTING_ALL, "none")[1]
    for i, f in enumerate(fl):                                   # the list the expected replacement starts from
        f.x, f.y, f.val = int(start["x"][i]), int(start["y"][i]), int(start["val"][i])
    sgf.KLTReplaceLostFeatures(tc, img, fl)
    check(_recs(fl), want_rep, "KLTReplaceLostFeatures")
    tc.selectionMask = None
    check(_recs(sgf.KLTSelectGoodFeatures(tc, img, n)), unmasked, "mask cleared")
    other = make_tc()                                            # another tracking context on the same device context: no mask
    tc.selectionMask = mask
    sgf.KLTSelectGoodFeatures(tc, img, n)
    check(_recs(sgf.KLTSelectGoodFeatures(other, img, n)), unmasked, "a tracking context without a mask after one with")


def test_track_sequence_under_a_mask_equals_the_host_loop():
    from pyfeaturetrack_amd import storeFeatures as sf, synth
    from pyfeaturetrack_amd.trackSequence import KLTTrackSequence
    sgf, tf = _api_modules()
    ncols, nrows, n, nf = 320, 240, 100, 6
    base = synth.synth_base(ncols, nrows, 17)
    frames = [synth.synth_frame(ncols, nrows, 17, k, shift=(1.3, -0.8), base=base) for k in range(nf)]
    frames[2] = frames[2].copy()
    frames[2][nrows // 8:nrows // 2, ncols // 8:ncols // 2] = 100            # features are lost here and replaced
    mask = rect_mask(ncols, nrows)
    rect = rect_of(ncols, nrows)

    def make():
        return make_tc(levels=2, ss=4, max_residue=10.0, sequentialMode=True, selectionMask=mask)
    tc = make()
    want = sf.KLTCreateFeatureTable(nf, n)
    fl = sgf.KLTSelectGoodFeatures(tc, frames[0], n)
    sf.KLTStoreFeatureList(fl, want, 0)
    replaced = 0
    for k in range(1, nf):
        tf.KLTTrackFeatures(tc, frames[k - 1], frames[k], fl)
        lost = np.array([f.val < 0 for f in fl])
        sgf.KLTReplaceLostFeatures(tc, frames[k], fl)
        new = _recs(fl)[lost]
        new = new[new["val"] >= 0]
        replaced += len(new)
        assert not inside_rect(new, rect).any(), "frame %d: a replacement placed a feature on a masked pixel" % k
        sf.KLTStoreFeatureList(fl, want, k)
    assert replaced > 0, "nothing was replaced: the clip shows nothing"
    assert not inside_rect(want.rec[0], rect).any()
    for kw in ({}, {"prefetch": False}, {"async_ingest": False}):
        got = KLTTrackSequence(make(), iter(frames), n, **kw)
        assert np.array_equal(got.val, want.val) and np.array_equal(got.x, want.x) and np.array_equal(got.y, want.y), kw
    plain = KLTTrackSequence(make_tc(levels=2, ss=4, max_residue=10.0, sequentialMode=True), iter(frames), n)
    assert not np.array_equal(plain.x, want.x), "the mask changes nothing on this clip"


# ---- 11: timing families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["all", "replace"])
def test_no_additional_launch_without_a_mask(mode):
    ncols, nrows = 322, 241
    start = expected(ncols, nrows, mode, "none")[0]

    def launches(g):
        g.c.timing_enable(1)                                     # (resets the figures)
        g.select(mode, start)
        counts = {t["name"]: t["launches"] for t in g.c.timing_read() if t["launches"]}
        g.c.timing_enable(0)
        return counts
    with Ctx(ncols, nrows) as g:
        g.select(mode, start)                                    # (first call: allocations; the number of passes enqueued before the
        before = launches(g)                                     # host looks follows what the previous selection needed)
        g.c.set_select_mask(rect_mask(ncols, nrows))
        masked = launches(g)
        g.c.set_select_mask(None)
        g.select(mode, start)                                    # (as before the first measurement)
        after = launches(g)
    assert after == before, (before, after)
    assert masked.get("seed_map", 0) == before.get("seed_map", 0) + 1, (before, masked)
