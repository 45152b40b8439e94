"""The selection-mask rule on the CPU oracle alone (no GPU), and the host-side pins of the feature."""
import os
import re

import numpy as np
import pytest

from helpers import make_tc, params_from_tc
from select_mask_expected import (REPLACING_SOME, drop_every_third, frame, inside_rect, rect_mask, rect_of, same_records,
                                  select_expected, window_mask)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("size", [(320, 240), (322, 241), (720, 480)], ids=lambda s: "%dx%d" % s)
def test_composition_without_a_mask_is_the_oracles_selection(size):
    """pins the helper: smooth, gradients, scan, sort and walk composed here are ko.select_good_features byte for byte, in both modes"""
    from oracle import klt_oracle as ko
    ncols, nrows = size
    p = params_from_tc(make_tc())
    n = 500 if ncols == 720 else 100
    img = frame(ncols, nrows).astype(np.float32)
    want = ko.select_good_features(p, img, n)
    got = select_expected(p, img, n)
    assert got.tobytes() == want.tobytes()
    start = drop_every_third(want)
    want2 = ko.select_good_features(p, img, n, mode=REPLACING_SOME, fl=start.copy())
    got2 = select_expected(p, img, n, mode=REPLACING_SOME, fl=start)
    assert got2.tobytes() == want2.tobytes()
    assert (start["val"] < 0).any() and (got2["val"] >= 0).all()


@pytest.mark.parametrize("size", [(320, 240), (322, 241), (720, 480)], ids=lambda s: "%dx%d" % s)
def test_rule_under_the_shared_masks(size):
    """what the GPU tests' inputs exercise: with the middle rectangle masked the list still fills and nothing lies inside it; with only a
    64 x 64 window allowed the candidates run out (27-30 features placed at these sizes)"""
    ncols, nrows = size
    p = params_from_tc(make_tc())
    n = 500 if ncols == 720 else 100
    img = frame(ncols, nrows).astype(np.float32)
    got = select_expected(p, img, n, mask=rect_mask(ncols, nrows))
    assert (got["val"] >= 0).all() and not inside_rect(got, rect_of(ncols, nrows)).any()
    assert not same_records(got, select_expected(p, img, n)), "the unmasked selection places nothing in the rectangle: the mask shows nothing"
    short = select_expected(p, img, n, mask=window_mask(ncols, nrows))
    placed = int((short["val"] >= 0).sum())
    print("%dx%d: %d features inside the 64x64 window" % (ncols, nrows, placed))
    assert 0 < placed < n
    assert (short["x"][placed:] == -1).all() and (short["val"][placed:] == -1).all()
    # a replacement keeps live features inside the masked rectangle and places none there
    full = select_expected(p, img, n)
    start = drop_every_third(full)
    live_inside = inside_rect(start, rect_of(ncols, nrows))
    assert live_inside.any()
    rep = select_expected(p, img, n, mode=REPLACING_SOME, fl=start, mask=rect_mask(ncols, nrows))
    assert np.array_equal(rep[start["val"] >= 0], start[start["val"] >= 0])
    assert not inside_rect(rep[start["val"] < 0], rect_of(ncols, nrows)).any()


def test_attribute_and_default():
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    from pyfeaturetrack_amd.params import selection_mask_from_tc
    tc = KLT_TrackingContext()
    assert tc.selectionMask is None
    assert selection_mask_from_tc(tc, 320, 240) is None

    class Foreign:                       # a context made elsewhere has no such field
        pass
    assert selection_mask_from_tc(Foreign(), 320, 240) is None


def test_accepted_values_become_bytes():
    from PIL import Image
    from pyfeaturetrack_amd.params import selection_mask_from_tc
    tc = make_tc()
    ref = rect_mask(32, 24)
    for given in (ref, ref.astype(bool), ref.astype(np.int64) * -7, ref.astype(np.uint16) * 256, ref.astype(np.int8) * -1,
                  Image.fromarray(ref * 255), Image.fromarray(ref * 255).convert("1"), np.asfortranarray(ref)):
        tc.selectionMask = given
        got = selection_mask_from_tc(tc, 32, 24)
        assert got.dtype == np.uint8 and got.shape == (24, 32) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got != 0, ref != 0)


@pytest.mark.parametrize("bad", [np.ones((240, 320), np.float32), [[1, 0], [0, 1]], "mask", np.ones((240, 320), object)],
                         ids=["float-array", "list", "str", "object-array"])
def test_wrong_type_raises_without_a_device(bad, monkeypatch):
    import pyfeaturetrack_amd.selectGoodFeatures as sgf
    import pyfeaturetrack_amd.trackSequence as seq
    sgf.KLT_verbose = 0
    _no_device(monkeypatch, sgf, seq)
    tc = make_tc(selectionMask=bad)
    img = np.zeros((240, 320), np.uint8)
    with pytest.raises(TypeError):
        sgf.KLTSelectGoodFeatures(tc, img, 10)
    with pytest.raises(TypeError):
        seq.KLTTrackSequence(tc, [img, img], 10)


def test_rgb_image_is_a_type_error(monkeypatch):
    from PIL import Image
    import pyfeaturetrack_amd.selectGoodFeatures as sgf
    import pyfeaturetrack_amd.trackSequence as seq
    sgf.KLT_verbose = 0
    _no_device(monkeypatch, sgf, seq)
    tc = make_tc(selectionMask=Image.new("RGB", (320, 240)))
    with pytest.raises(TypeError):
        sgf.KLTSelectGoodFeatures(tc, np.zeros((240, 320), np.uint8), 10)


@pytest.mark.parametrize("shape", [(241, 320), (240, 322), (320, 240), (240,), (2, 240, 320)], ids=str)
def test_wrong_shape_raises_without_a_device(shape, monkeypatch):
    import pyfeaturetrack_amd.selectGoodFeatures as sgf
    from pyfeaturetrack_amd.klt import KLT_Feature
    sgf.KLT_verbose = 0
    _no_device(monkeypatch, sgf)
    tc = make_tc(selectionMask=np.ones(shape, np.uint8))
    img = np.zeros((240, 320), np.uint8)
    with pytest.raises(ValueError):
        sgf.KLTSelectGoodFeatures(tc, img, 10)
    with pytest.raises(ValueError):
        sgf.KLTReplaceLostFeatures(tc, img, [KLT_Feature() for _ in range(4)])


def _no_device(monkeypatch, *modules):
    """any attempt to reach a device context fails the test"""
    def refuse(*a, **k):
        raise AssertionError("the call reached for a device context before it looked at tc.selectionMask")
    for m in modules:
        monkeypatch.setattr(m, "context_of", refuse)


def test_header_and_binding_carry_the_two_symbols():
    from pyfeaturetrack_amd import _abi
    header = open(os.path.join(REPO, "include", "klt_gpu.h")).read()
    assert re.search(r"int\s+klt_set_select_mask\(klt_ctx \*ctx, const uint8_t \*mask, int ncols, int nrows, int pitch\);", header)
    assert re.search(r"int\s+klt_set_select_mask_device\(klt_ctx \*ctx, const uint8_t \*dev_mask, int ncols, int nrows\);", header)
    assert re.search(r"#define KLT_ABI_VERSION 11\b", header)
    assert len(_abi.SYMBOLS["klt_set_select_mask"][1]) == 5 and len(_abi.SYMBOLS["klt_set_select_mask_device"][1]) == 4
    from pyfeaturetrack_amd.backend import Context
    for name in ("set_select_mask", "set_select_mask_device", "sync_select_mask"):
        assert callable(getattr(Context, name))


def test_printing_keeps_the_references_lines(capsys):
    from pyfeaturetrack_amd.klt import KLTPrintTrackingContext
    tc = make_tc(selectionMask=np.ones((4, 4), np.uint8))
    KLTPrintTrackingContext(tc)
    assert "selectionMask" not in capsys.readouterr().out
