"""The identity rule (include/klt_gpu.h, "track identities") on the host: the parameter function of the Python
layer, the numpy restatement (tests/reacquire_expected.py) against ident rows written out by hand on tables of 2 .. 5 slots, its
one-to-one assertion on 200 seeded draws, and the restatement against a plain per-slot loop on the same draws.  No GPU."""
import numpy as np
import pytest

import reacquire_expected as R
from helpers import make_tc

HAND = R.hand_cases()


def test_parameter_defaults():
    from pyfeaturetrack_amd.params import reacquire_params_from_tc
    tc = make_tc()
    assert reacquire_params_from_tc(tc) is None              # the switch is off by default
    assert reacquire_params_from_tc(object()) is None        # ... and a tracking context made elsewhere has none of the attributes
    tc.reacquireLost = True
    assert reacquire_params_from_tc(tc) == dict(capacity=1024, max_gap=30, max_distance=64, ratio_num=4, ratio_den=5, radius=24)
    assert R.reacquire_params_ok(**reacquire_params_from_tc(tc))
    tc.reacquire_radius, tc.reacquire_ratio, tc.reacquire_capacity, tc.reacquire_max_gap, tc.reacquire_max_distance = None, None, 1, 0, 256
    assert reacquire_params_from_tc(tc) == dict(capacity=1, max_gap=0, max_distance=256, ratio_num=0, ratio_den=1, radius=0)


@pytest.mark.parametrize("name, value, error", [
    ("reacquireLost", 1, ValueError), ("reacquireLost", "yes", ValueError),
    ("reacquire_capacity", 0, ValueError), ("reacquire_capacity", 3, ValueError), ("reacquire_capacity", 8192, ValueError),
    ("reacquire_capacity", 64.0, TypeError), ("reacquire_capacity", True, TypeError),
    ("reacquire_max_gap", -1, ValueError), ("reacquire_max_gap", 1.5, TypeError),
    ("reacquire_max_distance", 257, ValueError), ("reacquire_max_distance", -1, ValueError), ("reacquire_max_distance", 6.0, TypeError),
    ("reacquire_ratio", (5, 4), ValueError), ("reacquire_ratio", (0, 4), ValueError), ("reacquire_ratio", (1, 65536), ValueError),
    ("reacquire_ratio", 0.8, TypeError), ("reacquire_ratio", (1.0, 2), TypeError),
    ("reacquire_radius", -1, ValueError), ("reacquire_radius", 2.5, TypeError)])
def test_parameter_refusals(name, value, error):
    from pyfeaturetrack_amd.params import reacquire_params_from_tc
    tc = make_tc()
    tc.reacquireLost = True
    setattr(tc, name, value)
    with pytest.raises(error):
        reacquire_params_from_tc(tc)


def test_restatement_refuses_what_the_library_refuses():
    ok = dict(capacity=4, max_gap=0, max_distance=64, ratio_num=4, ratio_den=5, radius=0)
    assert R.reacquire_params_ok(**ok)
    for bad in (dict(capacity=0), dict(capacity=3), dict(capacity=8192), dict(max_gap=-1), dict(max_distance=257), dict(ratio_num=6),
                dict(radius=-1)):
        assert not R.reacquire_params_ok(**dict(ok, **bad)), bad


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    """every class of step 2, a refilled slot regaining its own id with gap 0, expiry at max_gap and max_gap + 1, L > C, ring wrap, two
    entries wanting one feature and two features wanting one entry on a flat frame (all distances tie), the gate at radius and radius + 1"""
    frames, lists, params, rows, (h, next_id, valid) = HAND[name]
    for cls in (R.Reacquire, R.ReacquireLoop):
        r = cls(**params)
        got = [r.begin(frames[0], lists[0])]
        for k in range(1, len(frames)):
            got.append(r.step(frames[k], lists[k], got[-1]))
        assert np.array_equal(np.stack(got), rows), (cls.__name__, np.stack(got).tolist())
        st = r.state()
        assert (int(st["k"]), int(st["h"]), int(st["next_id"]), int(st["valid"])) == (len(frames) - 1, h, next_id, valid), st


def test_hand_case_banks():
    """where the deposits of L > C and of a ring that wraps end up"""
    frames, lists, params, _, _ = HAND["more_lost_than_capacity"]
    r = R.Reacquire(**params)
    I = r.begin(frames[0], lists[0])
    r.step(frames[1], lists[1], I)
    assert r.bank["id"].tolist() == [2, 1] and r.bank["last_seen"].tolist() == [0, 0] and r.h == 1 and r.lost == 3
    frames, lists, params, _, _ = HAND["ring_wrap"]
    r = R.Reacquire(**params)
    I = r.begin(frames[0], lists[0])
    for k in (1, 2, 3):
        I = r.step(frames[k], lists[k], I)
    assert r.bank["id"].tolist() == [2, 1] and r.bank["last_seen"].tolist() == [2, 1] and r.h == 1


def test_ids_are_never_shared_within_a_row_on_200_draws():
    """the restatement asserts one-to-one inside every step (a fresh feature is taken by at most one bank entry); here also: no id twice
    in a row, a re-acquired id was alive before and is no id of the previous row, ids never exceed next_id"""
    reacquired = 0
    for seed in range(200):
        frames, lists, params = R.reacquire_draw(seed, small=seed >= 40)        # (the first 40 are the draws of the GPU test)
        rows, r = R.run_sequence(frames, lists, **params)
        seen = set()
        for k in range(len(rows)):
            ids = rows[k]["id"][rows[k]["val"] != 0]
            assert len(set(ids.tolist())) == len(ids), (seed, k)
            again = rows[k]["id"][rows[k]["val"] == R.REACQUIRED]
            assert set(again.tolist()) <= seen, (seed, k)
            if k:
                still = rows[k - 1]["id"][(rows[k - 1]["val"] != 0) & (rows[k]["val"] == R.CONTINUED)]
                assert not set(again.tolist()) & set(still.tolist()), (seed, k)
            reacquired += len(again)
            seen |= set(ids.tolist())
        assert max(seen, default=-1) < r.next_id
    assert reacquired > 200                                  # (the draws do exercise the match)


def test_restatement_equals_the_plain_loop_on_200_draws():
    for seed in range(200):
        frames, lists, params = R.reacquire_draw(seed, small=True)
        a, b = R.Reacquire(**params), R.ReacquireLoop(**params)
        Ia, Ib = a.begin(frames[0], lists[0]), b.begin(frames[0], lists[0])
        assert Ia.tobytes() == Ib.tobytes()
        for k in range(1, len(frames)):
            Ia, Ib = a.step(frames[k], lists[k], Ia), b.step(frames[k], lists[k], Ib)
            assert Ia.tobytes() == Ib.tobytes(), (seed, k, Ia.tolist(), Ib.tolist())
            assert a.bank.tobytes() == b.bank.tobytes() and a.state() == b.state(), (seed, k)
