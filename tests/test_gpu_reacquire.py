"""Track identities on the device (include/klt_gpu.h, "track identities") through the C ABI, against the rule in
numpy (tests/reacquire_expected.py): after every begin and every step the ident row, the downloaded bank and klt_reacquire_state equal
the restatement byte for byte.  Lists are uploaded with chosen val patterns and positions on 96 x 64 frames; no tracker is involved.
The lane, wavefront and chunk edges of the ranks, small banks, deposit counts around the capacity, fresh counts 0 / 1 / 65, every slot
lost and fresh at once, the hand cases, 40 seeded draws of six steps; the refusals; a context that never asks."""
import numpy as np
import pytest

import reacquire_expected as R

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = "error -1:", "error -3:"
FB_LIST, FB_IDENT = 200, (201, 202)


@pytest.fixture(scope="module")
def ctx():
    from pyfeaturetrack_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


def _check_against_the_rule(ctx, frames, lists, params, what):
    """runs the sequence on the device and in numpy side by side; returns the rows"""
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    params = dict(params)
    mode = params.pop("mode", R.UPRIGHT)
    r = R.Reacquire(mode=mode, **params)
    n = len(lists[0])
    ctx.set_descriptor_params(mode)
    ctx.set_reacquire_params(**{k: v for k, v in r.mp.items() if k != "cross_check"}, capacity=r.C, max_gap=r.max_gap)
    rows = []
    for k in range(len(frames)):
        ctx.upload(0, frames[k])
        ctx.featbuf_upload(FB_LIST, lists[k].astype(FEAT_DTYPE))
        cur, prev = FB_IDENT[k % 2], FB_IDENT[1 - k % 2]
        if k == 0:
            ctx.reacquire_begin_async(0, FB_LIST, cur, n)
            want = r.begin(frames[0], lists[0])
        else:
            ctx.reacquire_step_async(0, FB_LIST, prev, cur, n)
            want = r.step(frames[k], lists[k], rows[-1])
        got = ctx.ident_download(cur, n).view(R.IDENT_DTYPE)
        bad = np.flatnonzero([got[i].tobytes() != want[i].tobytes() for i in range(n)])
        assert not len(bad), "%s, step %d: %d of %d ident records differ; first %d: %r, the rule says %r" % (
            what, k, len(bad), n, bad[0], got[bad[0]], want[bad[0]])
        bank = ctx.reacquire_bank(r.C).view(R.BANK_DTYPE)
        badb = np.flatnonzero([bank[i].tobytes() != r.bank[i].tobytes() for i in range(r.C)])
        assert not len(badb), "%s, step %d: %d of %d bank entries differ; first %d: %r, the rule says %r" % (
            what, k, len(badb), r.C, badb[0], bank[badb[0]], r.bank[badb[0]])
        assert ctx.reacquire_state().tobytes() == r.state().tobytes(), (what, k, ctx.reacquire_state(), r.state())
        assert ctx.reacquire_path() == (2 if k == 0 else 5)
        rows.append(want)
    return np.stack(rows)


def _texture(seed=3):
    return np.random.default_rng(seed).integers(0, 256, R.FRAME_SHAPE, dtype=np.uint8)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_list_lengths_at_lane_wavefront_and_chunk_edges(ctx, n):
    """three steps of drawn lists at every list length where a rank crosses a lane mask, a wavefront or a chunk of 256, with banks of
    1, 2, 64 and 128 entries"""
    for C in (1, 2, 64, 128):
        rng = np.random.default_rng(n * 1000 + C)
        frame = _texture()
        lists = [R.draw_list(rng, n)]
        for k in range(3):
            lists.append(R.draw_list(rng, n, lists[-1], p_lost=0.4, p_refill=0.6))
        _check_against_the_rule(ctx, [frame] * 4, lists, dict(capacity=C, max_gap=1, radius=24), "n = %d, C = %d" % (n, C))


def _grid_list(n, val):
    """n records on distinct pixels of the 96 x 64 frame (a 13 x 10 grid for n <= 130), all of one val"""
    i = np.arange(n)
    return R.features(4 + 7 * (i % 13), 4 + 6 * (i // 13), np.full(n, val))


@pytest.mark.parametrize("lost", [0, 64, 65, 130], ids=lambda v: "L%d" % v)
@pytest.mark.parametrize("fresh", [0, 1, 65, 130], ids=lambda v: "fresh%d" % v)
def test_deposit_and_fresh_counts_around_the_capacity(ctx, lost, fresh):
    """130 slots, a bank of 64: L = 0, C, C + 1 and every slot; fresh count 0, 1, 65 and every slot -- with lost = fresh = 130 every slot
    is lost and fresh at once (the refilled slots come first, on their own corners: they regain their ids while the bank has room)"""
    n, C = 130, 64
    L0 = _grid_list(n, 7)
    L1 = _grid_list(n, 0)
    L1["val"][:lost] = -1                                    # the first `lost` slots are dropped ...
    both = min(lost, fresh)
    L1["val"][:both] = 9                                     # ... and `both` of them selected again on the spot
    if fresh > both:                                         # more fresh slots than lost ones: frame 0 had those slots empty
        L0["val"][n - (fresh - both):] = -1
        L1["val"][n - (fresh - both):] = 9
    L2 = L1.copy()
    L2["val"] = np.where(L1["val"] >= 0, 0, 5)               # next step: the dropped slots are selected again, one step late
    rows = _check_against_the_rule(ctx, [_texture()] * 3, [L0, L1, L2], dict(capacity=C, max_gap=3, radius=2), "L = %d, fresh = %d" % (lost, fresh))
    st = ctx.reacquire_state()
    assert int(st["k"]) == 2
    again = rows[1]["val"] == R.REACQUIRED
    # (the last C deposits survive: a slot selected again on the spot regains its id unless its deposit was overwritten)
    assert again.sum() == max(0, both - max(0, lost - C)) and np.array_equal(rows[1]["id"][again], np.flatnonzero(again))


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_cases_on_the_device(ctx, name):
    frames, lists, params, rows, _ = R.hand_cases()[name]
    got = _check_against_the_rule(ctx, frames, lists, params, name)
    assert np.array_equal(got, rows)


@pytest.mark.parametrize("seed", range(40))
def test_seeded_draws_of_six_steps(ctx, seed):
    frames, lists, params = R.reacquire_draw(seed)
    _check_against_the_rule(ctx, frames, lists, params, "draw %d" % seed)


def test_refusals_and_a_good_sequence_after_them(ctx):
    from pyfeaturetrack_amd._abi import KltBackendError
    from pyfeaturetrack_amd.backend import FEAT_DTYPE
    frames, lists, params, rows, _ = R.hand_cases()["classes"]
    n = len(lists[0])
    FB_VIEW, FB_SHORT, FB_NEW = 203, 204, 207
    ok = dict(capacity=4, max_gap=0, max_distance=64, ratio_num=4, ratio_den=5, radius=0)
    try:
        for bad in (dict(capacity=0), dict(capacity=3), dict(capacity=8192), dict(max_gap=-1), dict(max_distance=257), dict(max_distance=-1),
                    dict(ratio_num=6), dict(ratio_den=65536), dict(ratio_num=-1), dict(radius=-1)):
            with pytest.raises(KltBackendError, match=ERR_ARG):
                ctx.set_reacquire_params(**dict(ok, **bad))
        ctx.set_reacquire_params(**ok)                       # new parameters end whatever sequence an earlier test left
        ctx.upload(0, frames[0])
        ctx.upload(1, frames[0].astype(np.float32))
        ctx.slot_free(2)
        ctx.featbuf_upload(FB_LIST, lists[0].astype(FEAT_DTYPE))
        ctx.featbuf_upload(FB_SHORT, lists[0][:n - 1].astype(FEAT_DTYPE))
        ctx.featbuf_view(FB_VIEW, FB_LIST, 0, n)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_state()                            # nothing begun
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_bank(4)
        with pytest.raises(KltBackendError, match="error -3: klt_reacquire_step_async without"):
            ctx.reacquire_step_async(0, FB_LIST, FB_IDENT[0], FB_IDENT[1], n)
        with pytest.raises(KltBackendError, match="error -3: slot has no frame"):
            ctx.reacquire_begin_async(2, FB_LIST, FB_NEW, n)
        with pytest.raises(KltBackendError, match="error -3: slot has no frame"):
            ctx.reacquire_begin_async(7000, FB_LIST, FB_NEW, n)
        with pytest.raises(KltBackendError, match="error -3: descriptors take 8-bit frames"):
            ctx.reacquire_begin_async(1, FB_LIST, FB_NEW, n)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_begin_async(0, FB_LIST, FB_LIST, n)                    # aliasing by index
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_begin_async(0, FB_LIST, FB_VIEW, n)                    # ... and by address
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_begin_async(0, FB_LIST, FB_NEW, 0)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_begin_async(0, FB_LIST, -1, n)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_begin_async(0, FB_LIST, 29990, n)                      # the library's own descriptor buffers
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_begin_async(0, FB_SHORT, FB_NEW, n)               # the list is shorter
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_begin_async(0, 205, FB_NEW, n)                    # no such list
        assert ctx.featbuf_devptr(FB_NEW) is None       # no refused call allocated the row
        ctx.reacquire_begin_async(0, FB_LIST, FB_IDENT[0], n)
        with pytest.raises(KltBackendError, match="error -3: the feature count differs"):
            ctx.reacquire_step_async(0, FB_LIST, FB_IDENT[0], FB_IDENT[1], n - 1)
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_step_async(0, FB_LIST, FB_IDENT[0], FB_IDENT[0], n)    # the new row over the previous one
        with pytest.raises(KltBackendError, match=ERR_ARG):
            ctx.reacquire_step_async(0, FB_LIST, FB_IDENT[0], FB_VIEW, n)
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_step_async(0, FB_LIST, 206, FB_IDENT[1], n)            # no previous row
        with pytest.raises(KltBackendError, match=ERR_STATE):
            ctx.reacquire_step_async(0, FB_LIST, FB_SHORT, FB_IDENT[1], n)       # ... and a short one
        assert int(ctx.reacquire_state()["k"]) == 0          # no refused step counted
        ctx.set_reacquire_params(**ok)
        with pytest.raises(KltBackendError, match="error -3: klt_reacquire_step_async without"):
            ctx.reacquire_step_async(0, FB_LIST, FB_IDENT[0], FB_IDENT[1], n)    # new parameters ended the sequence
        got = _check_against_the_rule(ctx, frames, lists, params, "the good sequence after the refusals")
        assert np.array_equal(got, rows)
    finally:
        for k in range(3):
            ctx.slot_free(k)


def test_a_context_that_never_asks_reports_no_launch():
    from pyfeaturetrack_amd.backend import Context, FEAT_DTYPE
    c = Context(0)
    try:
        assert c.reacquire_path() == 0
        frame = _texture()
        feats = _grid_list(20, 3).astype(FEAT_DTYPE)
        c.upload(0, frame)
        c.timing_enable(True)
        c.describe(0, feats)                                 # the describe launch alone does not begin anything
        c.sync()
        assert c.reacquire_path() == 0
        assert not [t for t in c.timing_read() if t["name"].startswith("reacquire")]
    finally:
        c.close()
