"""The match launches on the device (include/klt_gpu.h, "descriptors", rule 2) against the rule in numpy
(tests/describe_expected.py), record for record: list lengths over the workgroup, tile and range edges, ties across them, undescribed
records, the distance, ratio and gate boundaries, the cross-check, bad parameters, seeded draws, and the golden pair's counts."""
import numpy as np
import pytest

import describe_expected as de
from conftest import GOLDEN, read_pgm

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = "error -1:", "error -3:"
DEFAULTS = dict(max_distance=64, ratio_num=4, ratio_den=5, cross_check=1, radius=0)


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _match(ctx, q, t, sync_entry=False, **params):
    p = dict(DEFAULTS)
    p.update(params)
    ctx.set_match_params(**p)
    return ctx.match(q, t, sync_entry=sync_entry).view(de.MATCH_DTYPE), de.match(q, t, **p)


def _same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.int32).reshape(-1, 4) != want.view(np.int32).reshape(-1, 4))
    if bad.size:
        i = int(bad[0]) // 4
        raise AssertionError("%s: %d of %d records differ; first %d: %r, the rule says %r" % (what, len(set((bad // 4).tolist())), len(want), i, got[i], want[i]))


@pytest.fixture(scope="module")
def pools():
    """1000 train and 257 query descriptors around a few centres, some undescribed, shared by the length table"""
    rng = np.random.default_rng(42)
    base = de.random_bases(rng, 6)
    return de.random_descriptors(rng, 257, spread=10, base=base), de.random_descriptors(rng, 1000, spread=10, base=base)


NQ = (0, 1, 2, 63, 64, 65, 255, 256, 257)
NT = (0, 1, 2, 255, 256, 257, 1000)


def test_list_lengths(ctx, pools):
    """every (nq, nt) of the table, cross-check and gate on and off by turns, both entry points"""
    q, t = pools
    seen = set()
    for a, nq in enumerate(NQ):
        for b, nt in enumerate(NT):
            params = dict(cross_check=(a + b) % 2, radius=(0, 80)[(a + 2 * b) % 2], ratio_num=(4, 0, 9)[(a + b) % 3], ratio_den=10)
            got, want = _match(ctx, q[:nq], t[:nt], sync_entry=bool((a * 7 + b) % 2), **params)
            _same_records(got, want, "nq %d, nt %d, %r" % (nq, nt, params))
            seen.update(want["val"].tolist())
            if nq:
                assert ctx.match_path() == de.splits_for(nq, nt)
            if nt == 0:
                assert (want["val"][q[:nq]["val"] == 1] == de.NO_CANDIDATE).all()
    assert seen == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("nq", [3, 257])
def test_best_and_second_in_different_ranges(ctx, nq):
    """1000 train records are cut into four ranges of a tile each: query i has its nearest record in one range and its second nearest in
    another, placed so that every pair of ranges occurs"""
    nt = 1000
    assert de.splits_for(nq, nt) == 4
    rng = np.random.default_rng(nq)
    t = np.zeros(nt, de.DESC_DTYPE)
    t["bits"] = rng.integers(0, 2 ** 32, (nt, 8), dtype=np.uint64).astype(np.uint32)
    t["val"] = 1
    q = np.zeros(nq, de.DESC_DTYPE)
    q["bits"] = rng.integers(0, 2 ** 32, (nq, 8), dtype=np.uint64).astype(np.uint32)
    q["val"] = 1
    taken = set()
    for i in range(min(nq, 12)):
        ra, rb = [(a, b) for a in range(4) for b in range(4) if a != b][i]
        ja, jb = ra * 256 + 17 + i, rb * 256 + 101 + i
        assert ja < nt and jb < nt and not {ja, jb} & taken
        taken |= {ja, jb}
        t["bits"][ja] = q["bits"][i]
        t["bits"][ja, 0] ^= np.uint32(1)                     # one bit away
        t["bits"][jb] = q["bits"][i]
        t["bits"][jb, 7] ^= np.uint32(0x00030000)            # two bits away
    got, want = _match(ctx, q, t, ratio_num=0, cross_check=1)
    assert ctx.match_path() == 4 > 1
    for i in range(min(nq, 12)):
        assert (want["distance"][i], want["second"][i]) == (1, 2) and want["train"][i] // 256 == [(a, b) for a in range(4) for b in range(4) if a != b][i][0]
    _same_records(got, want, "nq %d" % nq)
    got, want = _match(ctx, q, t, ratio_num=1, ratio_den=2, cross_check=0)      # 1 * 2 < 2 * 1 fails: the ratio sees the other range's second
    assert (want["val"][:min(nq, 12)] == de.AMBIGUOUS).all()
    _same_records(got, want, "nq %d, ratio 1/2" % nq)


def test_all_equal_descriptors(ctx):
    """every distance is 0: ties across tile and range edges go to the lowest index, in both directions"""
    q = np.zeros(130, de.DESC_DTYPE)
    t = np.zeros(1000, de.DESC_DTYPE)
    q["bits"] = t["bits"] = 0xDEADBEEF
    q["val"] = t["val"] = 1
    got, want = _match(ctx, q, t, ratio_num=0, cross_check=1)
    assert want["train"].tolist() == [0] * 130 and want["val"].tolist() == [de.MATCHED] + [de.NOT_MUTUAL] * 129 and (want["second"] == 0).all()
    _same_records(got, want, "all equal")
    t["val"][:700] = 0                                       # the first candidate lies in the third range
    q["val"][:70] = 0                                        # ... and the first described query in the second workgroup
    got, want = _match(ctx, q, t, ratio_num=0, cross_check=1)
    assert want["train"][70:].tolist() == [700] * 60 and want["val"][70] == de.MATCHED and (want["val"][:70] == 0).all()
    _same_records(got, want, "all equal, the first records undescribed")
    got, want = _match(ctx, q, t)                            # the ratio test on: 0 * 5 < 0 * 4 fails
    assert (want["val"][70:] == de.AMBIGUOUS).all()
    _same_records(got, want, "all equal, ratio on")


def test_undescribed_records_scattered(ctx):
    rng = np.random.default_rng(8)
    q, t = de.random_descriptors(rng, 200, centres=3), de.random_descriptors(rng, 900, centres=3)
    q["val"] = rng.random(200) < 0.5
    t["val"] = rng.random(900) < 0.3
    q["val"][q["val"] == 0] = rng.choice([0, 2, -1], int((q["val"] == 0).sum()))        # anything but 1 is "not described"
    t["val"][t["val"] == 0] = rng.choice([0, 2, -1], int((t["val"] == 0).sum()))
    for cross in (0, 1):
        got, want = _match(ctx, q, t, cross_check=cross, ratio_num=9, ratio_den=10)
        _same_records(got, want, "scattered, cross-check %d" % cross)
    t["val"] = 0
    got, want = _match(ctx, q, t)
    assert set(want["val"].tolist()) == {0, 2}
    _same_records(got, want, "no train record described")


def _flip(rec, nbits, start=0):
    out = rec.copy()
    for b in range(start, start + nbits):
        out["bits"][b >> 5] ^= np.uint32(1 << (b & 31))
    return out


def test_distance_and_ratio_boundaries(ctx):
    rng = np.random.default_rng(21)
    base = de.random_descriptors(rng, 1, spread=0, centres=1)[0]
    base["val"] = 1
    q = np.array([base], de.DESC_DTYPE)
    for d1, d2 in ((8, 10), (64, 80), (65, 256), (0, 0), (0, 1), (256, 256), (12, 15)):
        t = np.array([_flip(base, d2, 256 - d2), _flip(base, d1)], de.DESC_DTYPE)
        for max_distance in sorted({max(d1 - 1, 0), d1, min(d1 + 1, 256)}):
            for num, den in ((0, 1), (4, 5), (d1, d2) if 0 < d1 <= d2 else (1, 1), (d1 + 1, d2 + 1), (65535, 65535)):
                got, want = _match(ctx, q, t, max_distance=max_distance, ratio_num=num, ratio_den=den, cross_check=0)
                assert (want["train"][0], want["distance"][0], want["second"][0]) == (1 if d1 < d2 else 0, d1, d2)
                _same_records(got, want, "distances %d, %d; max %d; ratio %d / %d" % (d1, d2, max_distance, num, den))
    # the strict comparison: 8 * 5 == 10 * 4 fails, 8 passes under max_distance 8
    t = np.array([_flip(base, 10, 100), _flip(base, 8)], de.DESC_DTYPE)
    got, want = _match(ctx, q, t, max_distance=8, ratio_num=4, ratio_den=5, cross_check=0)
    assert tuple(got[0]) == (1, 8, 10, de.AMBIGUOUS)
    got, want = _match(ctx, q, t, max_distance=8, ratio_num=0, cross_check=0)
    assert tuple(got[0]) == (1, 8, 10, de.MATCHED)


def test_gate(ctx):
    rng = np.random.default_rng(22)
    base = de.random_bases(rng, 2)
    q = de.random_descriptors(rng, 70, base=base)
    t = de.random_descriptors(rng, 600, base=base)
    q["val"] = t["val"] = 1
    radius = 20
    # queries far from each other, every train record far from all of them -- but for the first 16 queries one record that lies exactly
    # `radius` away on one axis, or one pixel further
    q["cx"], q["cy"] = 1000 * np.arange(70), 500
    t["cx"] += 10 ** 6
    for i in range(8):
        off = (radius if i % 2 == 0 else radius + 1) * (1 if i % 4 < 2 else -1)
        t["cx"][300 + i], t["cy"][300 + i] = q["cx"][i] + off, q["cy"][i] - radius
        t["cx"][400 + i], t["cy"][400 + i] = q["cx"][i + 8] + radius, q["cy"][i + 8] + off
    got, want = _match(ctx, q, t, radius=radius, max_distance=256, ratio_num=0, cross_check=0)
    assert want["val"][:16].tolist() == [de.MATCHED if i % 2 == 0 else de.NO_CANDIDATE for i in range(16)]
    assert (want["val"][16:] == de.NO_CANDIDATE).all()
    _same_records(got, want, "radius %d" % radius)
    got, want = _match(ctx, q, t, radius=radius + 1, max_distance=256, ratio_num=0, cross_check=1)
    assert want["train"][:16].tolist() == list(range(300, 308)) + list(range(400, 408)) and (want["val"][:16] == de.MATCHED).all()
    _same_records(got, want, "radius %d" % (radius + 1))
    # a gate that lets several records through, with the ratio test and the cross-check behind it
    q["cx"], q["cy"] = rng.integers(0, 100, 70), rng.integers(0, 100, 70)
    t["cx"], t["cy"] = rng.integers(0, 100, 600), rng.integers(0, 100, 600)
    for r in (1, 7, 30, 200):
        got, want = _match(ctx, q, t, radius=r)
        _same_records(got, want, "radius %d on a crowded frame" % r)
    # centres anywhere in 32 bits
    q["cx"][:4] = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 5, -2 ** 31 + 3]
    t["cx"][:4] = [-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31]
    t["cy"][:4] = q["cy"][:4]
    got, want = _match(ctx, q, t, radius=2 ** 31 - 1, ratio_num=0, cross_check=0)
    _same_records(got, want, "the widest gate")
    got, want = _match(ctx, q, t, radius=4, max_distance=256, ratio_num=0, cross_check=0)
    assert want["train"][2] == 2 and want["train"][3] == 3 and want["val"][0] == de.NO_CANDIDATE
    _same_records(got, want, "gate at the ends of int32")


def test_cross_check_and_ratio_off(ctx, pools):
    q, t = pools
    q, t = q[:200], t[:700]
    for cross in (0, 1):
        for num in (0, 4):
            got, want = _match(ctx, q, t, cross_check=cross, ratio_num=num, max_distance=256)
            _same_records(got, want, "cross-check %d, ratio %d / 5" % (cross, num))
    on = de.match(q, t, cross_check=1, ratio_num=0, max_distance=256)
    off = de.match(q, t, cross_check=0, ratio_num=0, max_distance=256)
    assert (on["val"] == de.NOT_MUTUAL).any() and not (off["val"] == de.NOT_MUTUAL).any()
    # a set matched against itself: every described record is its own nearest neighbour at distance 0
    got, want = _match(ctx, t, t, cross_check=1, ratio_num=0)
    _same_records(got, want, "a set against itself")


def test_bad_parameters_and_buffers(ctx, pools):
    from pyfeaturetrack_amd._abi import KltBackendError
    q, t = pools
    _match(ctx, q[:5], t[:5])
    for bad in (dict(max_distance=257), dict(max_distance=-1), dict(ratio_num=6, ratio_den=5), dict(ratio_num=-1), dict(ratio_num=1, ratio_den=65536),
                dict(ratio_num=1, ratio_den=0), dict(cross_check=2), dict(cross_check=-1), dict(radius=-1)):
        p = dict(DEFAULTS)
        p.update(bad)
        assert not de.params_ok(**p)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.set_match_params(**p)
    for good in (dict(max_distance=0), dict(max_distance=256), dict(ratio_num=65535, ratio_den=65535), dict(ratio_num=0, ratio_den=-7), dict(radius=2 ** 31 - 1)):
        p = dict(DEFAULTS)
        p.update(good)
        ctx.set_match_params(**p)
    ctx.set_match_params(**DEFAULTS)
    FB_Q, FB_T, FB_M, FB_VIEW = 200, 201, 202, 203
    ctx.descriptor_upload(FB_Q, q[:64])
    ctx.descriptor_upload(FB_T, t[:300])
    ctx.featbuf_view(FB_VIEW, FB_T, 0, 64)
    ctx.timing_enable(True)
    try:
        for fb_match in (FB_Q, FB_T, FB_VIEW, -1):
            with pytest.raises(KltBackendError, match=ERR_ARG):
                ctx.match_async(FB_Q, 64, FB_T, 300, fb_match)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.match_async(FB_Q, -1, FB_T, 300, FB_M)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.match_async(FB_Q, 64, FB_T, -1, FB_M)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.match_async(FB_Q, 65, FB_T, 300, FB_M)      # the query buffer is shorter
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.match_async(FB_Q, 64, FB_T, 301, FB_M)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.match_async(FB_Q, 64, 204, 1, FB_M)          # no such buffer
        ctx.match_async(FB_Q, 0, FB_T, 300, FB_M)            # nq == 0: nothing to do
        ctx.sync()
        assert not [e for e in ctx.timing_read() if e["name"].startswith("match")]
        assert ctx.featbuf_devptr(FB_M) is None
        ctx.match_async(FB_Q, 64, FB_T, 300, FB_M)
        _same_records(ctx.featbuf_download(FB_M, 64).view(de.MATCH_DTYPE), de.match(q[:64], t[:300]), "the good call after the refusals")
        launches = {e["name"]: e["launches"] for e in ctx.timing_read()}
        assert (launches.get("match"), launches.get("match_resolve")) == (2, 1), launches      # forward, backward, resolve
        # the query set may be the train set
        ctx.match_async(FB_T, 300, FB_T, 300, FB_M)
        _same_records(ctx.featbuf_download(FB_M, 300).view(de.MATCH_DTYPE), de.match(t[:300], t[:300]), "fb_query == fb_train")
    finally:
        ctx.timing_enable(False)


def test_match_path_before_the_first_match():
    from pyfeaturetrack_amd._abi import KltBackendError
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    try:
        with pytest.raises(KltBackendError, match=ERR_STATE):
            c.match_path()
    finally:
        c.close()


def test_seeded_draws(ctx):
    seen = set()
    for seed in range(40):
        q, t, p = de.match_draw(seed)
        ctx.set_match_params(**p)
        got = ctx.match(q, t, sync_entry=bool(seed % 5 == 0)).view(de.MATCH_DTYPE)
        want = de.match(q, t, **p)
        _same_records(got, want, "draw %d: %d x %d, %r" % (seed, len(q), len(t), p))
        seen.update(want["val"].tolist())
    assert seen == {0, 1, 2, 3, 4, 5}


def test_golden_pair_counts_on_the_device(ctx):
    def describe(frame, feats, mode):
        ctx.upload(0, frame)
        ctx.set_descriptor_params(mode)
        return ctx.describe(0, feats).view(de.DESC_DTYPE)

    def match(q, t, radius):
        p = dict(DEFAULTS)
        p["radius"] = radius
        ctx.set_match_params(**p)
        return ctx.match(q, t).view(de.MATCH_DTYPE)
    try:
        de.check_golden_counts(de.golden_counts(describe, match, de.golden_pair(GOLDEN, read_pgm)))
    finally:
        ctx.slot_free(0)
