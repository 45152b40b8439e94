"""KLTDescribeFeatures / KLTMatchDescriptors against the rules in numpy (tests/describe_expected.py): numpy frames
and Pillow "L" images, the frame cache, the refusals, tc.descriptorOrientation, tc.equalization, and examples/reacquire.py."""
import os
import sys

import numpy as np
import pytest

import describe_expected as de
from conftest import GOLDEN, REPO, read_pgm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pair():
    return de.golden_pair(GOLDEN, read_pgm)


@pytest.fixture()
def quiet():
    from pyfeaturetrack_amd import selectGoodFeatures as sgf
    from pyfeaturetrack_amd import trackFeatures as tf
    old = sgf.KLT_verbose, tf.KLT_verbose
    sgf.KLT_verbose = tf.KLT_verbose = 0
    yield
    sgf.KLT_verbose, tf.KLT_verbose = old


def _tc(**attrs):
    from pyfeaturetrack_amd.klt import KLT_TrackingContext
    tc = KLT_TrackingContext()
    for k, v in attrs.items():
        setattr(tc, k, v)
    return tc


def _same(dl, want, what):
    got = dl.records.view(de.DESC_DTYPE)
    assert got.tobytes() == want.tobytes(), what
    assert np.array_equal(dl.bits, want["bits"].view(np.uint8).reshape(-1, 32)) and dl.bits.shape == (len(want), 32)
    assert np.array_equal(dl.val, want["val"]) and np.array_equal(dl.orientation, want["orientation"])
    assert np.array_equal(dl.x, want["cx"]) and np.array_equal(dl.y, want["cy"]) and len(dl) == len(want)


def test_describe_and_match_equal_the_rules(pair, quiet):
    from PIL import Image
    import pyfeaturetrack_amd as klt
    img0, img1, f0, f1 = pair
    tc = _tc()
    fl = klt.KLTSelectGoodFeatures(tc, img0, 100)
    rec = klt.selectGoodFeatures.features_to_array(fl).copy().view(de.FEAT_DTYPE)
    for toggle in (False, True, False):                      # tc.descriptorOrientation toggled between calls
        tc.descriptorOrientation = toggle
        mode = de.STEERED if toggle else de.UPRIGHT
        want0, want1 = de.describe(img0, rec, mode), de.describe(img1, f1, mode)
        d0 = klt.KLTDescribeFeatures(tc, img0, fl)                                       # a feature list on a numpy frame
        _same(d0, want0, "feature list, numpy frame, orientation %s" % toggle)
        d0p = klt.KLTDescribeFeatures(tc, Image.fromarray(img0), rec)                    # a record array on a Pillow "L" image
        _same(d0p, want0, "record array, Pillow image, orientation %s" % toggle)
        d1 = klt.KLTDescribeFeatures(tc, Image.fromarray(img1), f1.view(klt.describeFeatures.FEAT_DTYPE))
        _same(d1, want1, "tracked records, Pillow image, orientation %s" % toggle)
        assert isinstance(d0, klt.KLT_DescriptorList) and (want0["orientation"] == 0).all() != toggle
        for kw, ref in ((dict(), dict()), (dict(ratio=None, cross_check=False), dict(ratio_num=0, cross_check=0)),
                        (dict(max_distance=30, ratio=(9, 10), radius=20), dict(max_distance=30, ratio_num=9, ratio_den=10, radius=20)),
                        (dict(radius=0), dict(radius=0))):
            m = klt.KLTMatchDescriptors(tc, d0, d1, **kw)
            assert m.dtype.names == ("train", "distance", "second", "val")
            assert m.view(de.MATCH_DTYPE).tobytes() == de.match(want0, want1, **ref).tobytes(), (toggle, kw)
        m = klt.KLTMatchDescriptors(tc, d0.records, d1[np.arange(50)])                   # record arrays and sub-lists
        assert m.view(de.MATCH_DTYPE).tobytes() == de.match(want0, want1[:50]).tobytes()
        assert len(klt.KLTMatchDescriptors(tc, d0[:0], d1)) == 0
    assert len(klt.KLTDescribeFeatures(tc, img0, rec[:0])) == 0


def test_cached_frame_is_not_uploaded_again(pair, quiet):
    import pyfeaturetrack_amd as klt
    from pyfeaturetrack_amd.backend import context_of
    img0, img1, _, _ = pair
    tc = _tc()
    fl = klt.KLTSelectGoodFeatures(tc, img0, 60)
    klt.KLTTrackFeatures(tc, img0, img1, fl)
    ctx = context_of(tc)
    calls = []
    for name in ("upload", "upload_async"):
        real = getattr(ctx, name)
        setattr(ctx, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    try:
        rec = klt.selectGoodFeatures.features_to_array(fl).copy().view(de.FEAT_DTYPE)
        for img in (img0, img1):
            assert klt.KLTDescribeFeatures(tc, img, fl).records.view(de.DESC_DTYPE).tobytes() == de.describe(img, rec).tobytes()
        assert calls == []
        other = np.ascontiguousarray(img0[::-1])
        assert klt.KLTDescribeFeatures(tc, other, fl).records.view(de.DESC_DTYPE).tobytes() == de.describe(other, rec).tobytes()
        assert len(calls) == 1                               # a frame no slot holds goes to the selection's own slot ...
        klt.KLTTrackFeatures(tc, img0, img1, fl)
        assert len(calls) == 1                               # ... and the pair's two frames are still where they were
    finally:
        for name in ("upload", "upload_async"):
            delattr(ctx, name)


def test_value_errors_come_before_the_device(pair):
    from PIL import Image
    import pyfeaturetrack_amd as klt
    img0, _, f0, _ = pair
    rec = f0.view(klt.describeFeatures.FEAT_DTYPE)
    tc = _tc()
    for bad in (img0.astype(np.float32), np.dstack([img0] * 3), Image.fromarray(img0).convert("RGB"), Image.fromarray(img0).convert("F")):
        with pytest.raises(ValueError, match="descriptors take single-channel 8-bit frames"):
            klt.KLTDescribeFeatures(tc, bad, rec)
    tc.descriptorOrientation = 1
    with pytest.raises(ValueError, match="descriptorOrientation"):
        klt.KLTDescribeFeatures(tc, img0, rec)
    tc.descriptorOrientation = False
    with pytest.raises(TypeError):
        klt.KLTDescribeFeatures(tc, img0, rec.view(np.uint8))
    d = klt.KLT_DescriptorList(de.describe(img0, f0[:5]))
    for kw, err in ((dict(max_distance=257), ValueError), (dict(max_distance=-1), ValueError), (dict(max_distance=6.5), TypeError),
                    (dict(ratio=(5, 4)), ValueError), (dict(ratio=(0, 4)), ValueError), (dict(ratio=(1, 65536)), ValueError),
                    (dict(ratio=0.8), TypeError), (dict(ratio=(1.0, 2)), TypeError), (dict(cross_check=1), TypeError),
                    (dict(radius=-1), ValueError), (dict(radius=2.5), TypeError)):
        with pytest.raises(err):
            klt.KLTMatchDescriptors(tc, d, d, **kw)
    with pytest.raises(TypeError):
        klt.KLTMatchDescriptors(tc, d, np.zeros(3))
    assert "_klt_ctx" not in tc.__dict__                     # no device context was asked for


def test_equalization_is_honoured(pair, quiet):
    import pyfeaturetrack_amd as klt
    img0, _, f0, _ = pair
    rec = f0.view(klt.describeFeatures.FEAT_DTYPE)
    dark = img0.copy()
    dark[:, :160] = dark[:, :160] // 5
    on, off = _tc(equalization="clahe"), _tc()
    seen = klt.KLTEqualizeImage(off, dark)
    assert not np.array_equal(seen, dark)
    got = klt.KLTDescribeFeatures(on, dark, rec)
    ref = klt.KLTDescribeFeatures(off, seen, rec)
    assert got.records.tobytes() == ref.records.tobytes() == de.describe(seen, f0).tobytes()
    assert got.records.tobytes() != klt.KLTDescribeFeatures(off, dark, rec).records.tobytes()
    with pytest.raises(ValueError):
        klt.KLTDescribeFeatures(_tc(equalization="clahe", clahe_tiles=(64, 64)), dark[:40, :40], rec)


def test_reacquire_example(quiet):
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import reacquire
        results = reacquire.main(["--size", "256x192", "--features", "300", "--frames", "20", "--cover", "4:12"])
    finally:
        sys.path.pop(0)
    (alive_off, regained_off, _, lost_off), (alive_on, regained_on, wrong_on, lost_on) = results[False], results[True]
    assert regained_off == 0 and lost_off > 10 and lost_on > 10
    assert alive_on > alive_off and regained_on >= alive_on - alive_off > 0
    assert wrong_on * 10 <= regained_on                      # the descriptor and the gate find the corner itself
