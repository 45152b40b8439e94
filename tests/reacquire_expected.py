"""The identity rule of include/klt_gpu.h, "track identities" (DESIGN.md section 9o), restated in numpy: every slot of every frame gets a
persistent track id, lost tracks leave descriptor and id in a ring bank, newly selected features are matched against the bank and inherit
the old id on a mutual match.  Steps 1 and 5 are `describe` and `match` of tests/describe_expected.py.  The device output (ident rows,
bank, state) equals what stands here byte for byte.  Also a plain per-slot loop of the same rule and the seeded trials of the GPU tests."""
import numpy as np

from describe_expected import (DESC_DTYPE, FEAT_DTYPE, MATCHED, UPRIGHT, describe, distances, features, match, params_ok)

IDENT_DTYPE = np.dtype([("id", np.int32), ("gap", np.int32), ("distance", np.int32), ("val", np.int32)])
BANK_DTYPE = np.dtype([("d", DESC_DTYPE), ("id", np.int32), ("last_seen", np.int32), ("valid", np.int32), ("pad", np.int32)])
STATE_DTYPE = np.dtype([(k, np.int32) for k in ("k", "h", "next_id", "valid", "fresh", "lost")])
assert IDENT_DTYPE.itemsize == 16 and BANK_DTYPE.itemsize == 64 and STATE_DTYPE.itemsize == 24

NO_TRACK, CONTINUED, NEW, REACQUIRED = 0, 1, 2, 3          # klt_ident.val
MAX_CAPACITY = 4096


def reacquire_params_ok(capacity, max_gap, max_distance, ratio_num, ratio_den, radius):
    return (1 <= capacity <= MAX_CAPACITY and capacity & (capacity - 1) == 0 and max_gap >= 0
            and params_ok(max_distance, ratio_num, ratio_den, 1, radius))


class Reacquire:
    """the state of one context: begin(frame, L0) -> I0, step(frame, Lk, I(k-1)) -> Ik"""

    def __init__(self, capacity=1024, max_gap=30, max_distance=64, ratio_num=4, ratio_den=5, radius=24, mode=UPRIGHT):
        assert reacquire_params_ok(capacity, max_gap, max_distance, ratio_num, ratio_den, radius)
        self.C, self.max_gap, self.mode = capacity, max_gap, mode
        self.mp = dict(max_distance=max_distance, ratio_num=ratio_num, ratio_den=ratio_den, cross_check=1, radius=radius)
        self.n = None

    def begin(self, frame, L):
        n = len(L)
        I = np.zeros(n, IDENT_DTYPE)
        live = L["val"] >= 0
        I["id"] = np.where(live, np.arange(n), -1)
        I["val"] = np.where(live, NEW, NO_TRACK)
        self.n, self.k, self.h, self.next_id = n, 0, 0, n
        self.bank = np.zeros(self.C, BANK_DTYPE)
        self.P = describe(frame, L, self.mode)
        self.fresh = self.lost = 0
        return I

    def step(self, frame, L, Iprev):
        assert self.n == len(L) == len(Iprev)
        C, bank, P = self.C, self.bank, self.P
        k = self.k + 1
        Q = describe(frame, L, self.mode)                                                   # 1
        had = Iprev["val"] != 0                                                             # 2
        cont = had & (L["val"] == 0)
        fresh = (L["val"] >= 0) & ~cont
        lost = had & ~cont
        bank[(bank["valid"] == 1) & (k - bank["last_seen"].astype(np.int64) - 1 > self.max_gap)] = 0      # 3 (a cleared entry is all zero)
        dep = np.flatnonzero(lost & (P["val"] == 1))                                        # 4
        for r, s in enumerate(dep):                          # (all of them in order: the outcome the rule asks for when L > C)
            e = bank[(self.h + r) & (C - 1)]
            e["d"], e["id"], e["last_seen"], e["valid"], e["pad"] = P[s], Iprev["id"][s], k - 1, 1, 0
        self.h = (self.h + len(dep)) & (C - 1)
        q = bank["d"].copy()                                                                # 5
        q["val"][bank["valid"] != 1] = 0
        fs = np.flatnonzero(fresh)
        m = match(q, Q[fs], **self.mp)
        I = np.zeros(self.n, IDENT_DTYPE)                                                   # 6
        I["id"] = -1
        hit = np.flatnonzero(m["val"] == MATCHED)
        trains = m["train"][hit]
        # the cross-check makes the assignment one-to-one: bank entry i is matched only when train record j's own best query is i, and
        # that best query is one value per j -- two entries cannot both be it.  (One train per query holds for any match.)
        assert len(set(trains.tolist())) == len(trains), "two bank entries took one fresh feature"
        taken = np.zeros(self.n, bool)
        for i, j in zip(hit, trains):
            s = fs[j]
            I[s] = (bank["id"][i], k - bank["last_seen"][i] - 1, m["distance"][i], REACQUIRED)
            taken[s] = True
            bank[i] = 0
        new = np.flatnonzero(fresh & ~taken)
        I["id"][new] = self.next_id + np.arange(len(new))
        I["val"][new] = NEW
        self.next_id += len(new)
        I["id"][cont] = Iprev["id"][cont]
        I["val"][cont] = CONTINUED
        self.P, self.k, self.fresh, self.lost = Q, k, len(fs), len(dep)                     # 7
        return I

    def state(self):
        out = np.zeros((), STATE_DTYPE)
        out["k"], out["h"], out["next_id"] = self.k, self.h, self.next_id
        out["valid"], out["fresh"], out["lost"] = int((self.bank["valid"] == 1).sum()), self.fresh, self.lost
        return out


# ---- the same rule as a plain loop over slots, bank entries and descriptor pairs (no describe_expected.match)
def _popcount(a, b):
    return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))


class ReacquireLoop(Reacquire):
    def step(self, frame, L, Iprev):
        C, bank, P, mp = self.C, self.bank, self.P, self.mp
        k = self.k + 1
        Q = describe(frame, L, self.mode)
        I = np.zeros(self.n, IDENT_DTYPE)
        for i in range(C):
            if bank["valid"][i] == 1 and k - int(bank["last_seen"][i]) - 1 > self.max_gap:
                bank[i] = 0
        fs, nlost = [], 0
        for s in range(self.n):
            had = Iprev["val"][s] != 0
            cont = had and L["val"][s] == 0
            if had and not cont and P["val"][s] == 1:
                e = bank[(self.h + nlost) & (C - 1)]
                e["d"], e["id"], e["last_seen"], e["valid"], e["pad"] = P[s], Iprev["id"][s], k - 1, 1, 0
                nlost += 1
            if L["val"][s] >= 0 and not cont:
                fs.append(s)
            I[s] = (Iprev["id"][s], 0, 0, CONTINUED) if cont else (-1, 0, 0, NO_TRACK)
        self.h = (self.h + nlost) & (C - 1)

        def cand(i, s):
            if bank["valid"][i] != 1 or bank["d"]["val"][i] != 1 or Q["val"][s] != 1:
                return False
            r = mp["radius"]
            return r == 0 or (abs(int(bank["d"]["cx"][i]) - int(Q["cx"][s])) <= r and abs(int(bank["d"]["cy"][i]) - int(Q["cy"][s])) <= r)
        d = {(i, s): _popcount(bank["d"]["bits"][i], Q["bits"][s]) for i in range(C) for s in fs if cand(i, s)}
        adopted = {}
        for i in range(C):
            mine = sorted((d[i, s], s) for s in fs if (i, s) in d)
            if not mine:
                continue
            dist, s = mine[0]
            second = mine[1][0] if len(mine) > 1 else 257
            if dist > mp["max_distance"] or (mp["ratio_num"] and not dist * mp["ratio_den"] < second * mp["ratio_num"]):
                continue
            if min((d[j, s], j) for j in range(C) if (j, s) in d)[1] != i:
                continue
            assert s not in adopted
            adopted[s] = i
        for s, i in adopted.items():
            I[s] = (bank["id"][i], k - int(bank["last_seen"][i]) - 1, d[i, s], REACQUIRED)
            bank[i] = 0
        for s in fs:
            if s not in adopted:
                I[s] = (self.next_id, 0, 0, NEW)
                self.next_id += 1
        self.P, self.k, self.fresh, self.lost = Q, k, len(fs), nlost
        return I


def run_sequence(frames, lists, **params):
    """the ident rows of a whole [frame][slot] table of FEAT_DTYPE records on its frames"""
    r = Reacquire(**params)
    rows = [r.begin(frames[0], lists[0])]
    for k in range(1, len(frames)):
        rows.append(r.step(frames[k], lists[k], rows[-1]))
    return np.stack(rows), r


# ---- seeded trials
FRAME_SHAPE = (64, 96)                                       # nrows, ncols


def draw_list(rng, n, prev=None, p_lost=0.25, p_refill=0.5, flat=False):
    """a list as a tracker and a replacement pass leave it: tracked slots (val 0) moved a little, lost ones (val < 0), refilled and
    newly selected ones (val > 0)"""
    nrows, ncols = FRAME_SHAPE
    f = np.zeros(n, FEAT_DTYPE)
    if prev is None:
        f["x"] = rng.uniform(0, ncols - 1, n).astype(np.float32)
        f["y"] = rng.uniform(0, nrows - 1, n).astype(np.float32)
        f["val"] = np.where(rng.random(n) < 0.8, rng.integers(1, 5000, n), -1)
        return f
    f["x"] = prev["x"] + rng.uniform(-1.5, 1.5, n).astype(np.float32)
    f["y"] = prev["y"] + rng.uniform(-1.5, 1.5, n).astype(np.float32)
    alive = prev["val"] >= 0
    lose = rng.random(n) < p_lost
    f["val"] = np.where(alive & ~lose, 0, rng.integers(-5, 0, n))
    refill = (f["val"] < 0) & (rng.random(n) < p_refill)
    k = int(refill.sum())
    # a refilled slot: near where some feature stood before (so that the bank has something to find), or anywhere
    src = rng.integers(0, n, k)
    near = rng.random(k) < 0.7
    f["x"][refill] = np.where(near, prev["x"][src] + rng.integers(-2, 3, k), rng.uniform(0, ncols - 1, k)).astype(np.float32)
    f["y"][refill] = np.where(near, prev["y"][src] + rng.integers(-2, 3, k), rng.uniform(0, nrows - 1, k)).astype(np.float32)
    f["val"][refill] = rng.integers(1, 5000, k)
    f["aux"] = rng.integers(-3, 3, n)
    return f


def reacquire_draw(seed, small=False):
    """one seeded trial of six steps: (frames [7], lists [7], parameters); small: lists and banks a plain Python loop gets through"""
    rng = np.random.default_rng(4100 + seed)
    n = int(rng.choice([1, 3, 5, 12, 30] if small else [1, 3, 5, 40, 63, 64, 65, 130, 257]))
    kind = seed % 5
    frames = []
    base = rng.integers(0, 256, FRAME_SHAPE, dtype=np.uint8)
    for k in range(7):
        if kind == 0:                                        # a flat frame: every descriptor equal, ties everywhere
            frames.append(np.full(FRAME_SHAPE, 90, np.uint8))
        elif kind == 1:                                      # new noise every frame: nothing is found again
            frames.append(rng.integers(0, 256, FRAME_SHAPE, dtype=np.uint8))
        else:                                                # one texture, a few pixels changed per frame
            fr = base.copy()
            idx = rng.integers(0, fr.size, fr.size // 50)
            fr.reshape(-1)[idx] = rng.integers(0, 256, len(idx), dtype=np.uint8)
            frames.append(fr)
    lists = [draw_list(rng, n)]
    for k in range(1, 7):
        lists.append(draw_list(rng, n, lists[-1], p_lost=float(rng.choice([0.0, 0.1, 0.3, 1.0])), p_refill=float(rng.choice([0.0, 0.5, 1.0]))))
    den = int(rng.integers(1, 65536))
    params = dict(capacity=int(rng.choice([1, 2, 4, 16, 32] if small else [1, 2, 4, 16, 64, 128, 1024])), max_gap=int(rng.choice([0, 1, 2, 30])),
                  max_distance=int(rng.choice([0, 16, 64, 128, 256])), ratio_num=int(rng.integers(1, den + 1)) if seed % 3 else 0,
                  ratio_den=den, radius=int(rng.choice([0, 3, 24, 500])), mode=UPRIGHT + (seed // 5) % 2)
    return frames, lists, params


# ---- the hand cases: (frames, lists, parameters, expected ident rows written out by hand, expected (h, next_id, valid) at the end)
def _texture():
    return np.random.default_rng(77).integers(0, 256, FRAME_SHAPE, dtype=np.uint8)


def _flat():
    return np.full(FRAME_SHAPE, 120, np.uint8)


# corners far apart (more than any radius used below) on the 96 x 64 frame
A, B, C_, D, E, F = (10, 10), (80, 10), (10, 50), (80, 50), (45, 30), (45, 8)
_OFF = dict(max_distance=256, ratio_num=0, ratio_den=1)     # only the gate and the cross-check decide


def _lst(*slots):
    """slots: (position, val) pairs"""
    return features([p[0] for p, _ in slots], [p[1] for p, _ in slots], [v for _, v in slots])


def _rows(*rows):
    return np.array([[tuple(r) for r in row] for row in rows], IDENT_DTYPE)


_N = (-1, 0, 0, 0)


def hand_cases():
    tex, flat = _texture(), _flat()
    cases = {}
    # every class of step 2: continued, lost without refill, fresh in an empty slot, refilled (lost and fresh) far from where it was
    cases["classes"] = ([tex] * 2, [_lst((A, 5), (B, 7), (C_, -1), (D, 9)), _lst((A, 0), (B, -2), (E, 3), (F, 8))], dict(capacity=4),
                        _rows([(0, 0, 0, 2), (1, 0, 0, 2), _N, (3, 0, 0, 2)], [(0, 0, 0, 1), _N, (4, 0, 0, 2), (5, 0, 0, 2)]), (2, 6, 2))
    # a slot the tracker dropped and the replacement pass selected again on the same corner: its own id, gap 0
    cases["refill_same_corner"] = ([tex] * 2, [_lst((A, 5), (B, 7), (C_, 9)), _lst((A, 0), (B, 4), (C_, 0))], dict(capacity=4),
                                   _rows([(0, 0, 0, 2), (1, 0, 0, 2), (2, 0, 0, 2)], [(0, 0, 0, 1), (1, 0, 0, 3), (2, 0, 0, 1)]), (1, 3, 0))
    # lost at step 1 (last seen in frame 0), selected again at step 3: gap 2 -- inside max_gap = 2, expired under max_gap = 1
    seq = [_lst((A, 5), (B, 7)), _lst((A, 0), (B, -1)), _lst((A, 0), (B, -1)), _lst((A, 0), (B, 6))]
    head = [[(0, 0, 0, 2), (1, 0, 0, 2)], [(0, 0, 0, 1), _N], [(0, 0, 0, 1), _N]]
    cases["gap_at_max"] = ([tex] * 4, seq, dict(capacity=2, max_gap=2), _rows(*head, [(0, 0, 0, 1), (1, 2, 0, 3)]), (1, 2, 0))
    cases["gap_past_max"] = ([tex] * 4, seq, dict(capacity=2, max_gap=1), _rows(*head, [(0, 0, 0, 1), (2, 0, 0, 2)]), (1, 3, 0))
    # L > C: three deposits into a bank of two -- the last two stay, slot 1's at position 1, slot 2's at position 0; slot 0's is gone,
    # so at step 2 corner A is new while B and C_ come back
    cases["more_lost_than_capacity"] = ([tex] * 3, [_lst((A, 5), (B, 7), (C_, 9)), _lst((A, -1), (B, -1), (C_, -1)), _lst((A, 3), (B, 3), (C_, 3))],
                                        dict(capacity=2), _rows([(0, 0, 0, 2), (1, 0, 0, 2), (2, 0, 0, 2)], [_N, _N, _N],
                                                                [(3, 0, 0, 2), (1, 1, 0, 3), (2, 1, 0, 3)]), (1, 4, 0))
    # ring wrap across steps: one deposit per step into a bank of two; the third overwrites the first
    cases["ring_wrap"] = ([tex] * 5, [_lst((A, 5), (B, 7), (C_, 9)), _lst((A, -1), (B, 0), (C_, 0)), _lst((A, -1), (B, -1), (C_, 0)),
                                      _lst((A, -1), (B, -1), (C_, -1)), _lst((A, 2), (B, 2), (C_, 2))], dict(capacity=2),
                          _rows([(0, 0, 0, 2), (1, 0, 0, 2), (2, 0, 0, 2)], [_N, (1, 0, 0, 1), (2, 0, 0, 1)], [_N, _N, (2, 0, 0, 1)], [_N, _N, _N],
                                [(3, 0, 0, 2), (1, 2, 0, 3), (2, 1, 0, 3)]), (1, 4, 0))
    # a flat frame: every descriptor equal, every distance 0.  Two bank entries, three fresh slots: both entries' best is the lowest
    # fresh slot (slot 0... here slot 2), whose best query is the lowest bank position; the other entry is not mutual and stays
    cases["ties_two_entries_one_feature"] = ([flat] * 2, [_lst((A, 5), (B, 7), (C_, -1), (D, -1), (E, -1)), _lst((A, -1), (B, -1), (C_, 1), (D, 1), (E, 1))],
                                             dict(capacity=4, radius=0, **_OFF),
                                             _rows([(0, 0, 0, 2), (1, 0, 0, 2), _N, _N, _N], [_N, _N, (0, 0, 0, 3), (5, 0, 0, 2), (6, 0, 0, 2)]), (2, 7, 1))
    # ... and two fresh features wanting one bank entry: the lower slot gets it
    cases["ties_two_features_one_entry"] = ([flat] * 2, [_lst((A, 5), (B, -1), (C_, -1)), _lst((A, -1), (B, 1), (C_, 1))], dict(capacity=4, radius=0, **_OFF),
                                            _rows([(0, 0, 0, 2), _N, _N], [_N, (0, 0, 0, 3), (3, 0, 0, 2)]), (1, 4, 0))
    # the gate on the flat frame: 5 pixels away with radius 5 is a candidate, 6 pixels away is not
    for name, dx, row in (("gate_at_radius", 5, [_N, (0, 0, 0, 3)]), ("gate_past_radius", 6, [_N, (2, 0, 0, 2)])):
        cases[name] = ([flat] * 2, [_lst((A, 5), (B, -1)), _lst((A, -1), ((A[0] + dx, A[1] - dx if dx == 5 else A[1]), 1))], dict(capacity=4, radius=5, **_OFF),
                       _rows([(0, 0, 0, 2), _N], row), (1, 2 if dx == 5 else 3, 0 if dx == 5 else 1))
    return cases


# ---- the clip of the API tests: the drifting scene of examples/reacquire.py with a flat block over its middle for some frames
CLIP_SHIFT = (1.0, 0.5)                                      # the scene's motion, pixels per frame


def occluded_clip(w=160, h=120, frames=12, cover=(3, 8), seed=17):
    from pyfeaturetrack_amd import synth
    base = synth.synth_base(w, h, seed)
    clip = [synth.shift_frame(base, k * CLIP_SHIFT[0], k * CLIP_SHIFT[1]) for k in range(frames)]
    for k in range(cover[0], min(cover[1], frames)):
        clip[k][h // 4: 3 * h // 4, w // 3: 2 * w // 3] = 128
    return clip


def oracle_lists(p, clip, n, replace_lost=True):
    """the [frame][slot] lists the CPU oracle produces for the clip: select, then per frame track and (replace_lost) replace"""
    from oracle import klt_oracle as ko
    f_prev = clip[0].astype(np.float32)
    fl = ko.select_good_features(p, f_prev, n)
    rows = [fl.copy()]
    P_prev = ko.Pyramids(p, f_prev)
    for k in range(1, len(clip)):
        f = clip[k].astype(np.float32)
        P_cur = ko.Pyramids(p, f)
        ko.track_features(p, P_prev, P_cur, fl)
        if replace_lost:
            fl = ko.select_good_features(p, f, n, mode=2, fl=fl)
        rows.append(fl.copy())
        P_prev = P_cur
    return np.stack(rows)


def clip_counts(lists, ident, n, wrong_px=2.0):
    """(identities of frame 0 alive in the last frame; of them, re-acquired on the way; of those, sitting more than wrong_px from the
    corner the identity began on, the scene motion being known; the largest gap of any re-acquisition)"""
    last = len(lists) - 1
    again = set(int(i) for i in ident["id"][ident["val"] == REACQUIRED])
    alive = [(s, int(i)) for s, i in enumerate(ident[last]["id"]) if ident[last]["val"][s] != 0 and 0 <= i < n]
    regained = [(s, i) for s, i in alive if i in again]
    wrong = 0
    for s, i in regained:                                    # identity i began in slot i of frame 0
        dx = lists[last]["x"][s] - last * CLIP_SHIFT[0] - lists[0]["x"][i]
        dy = lists[last]["y"][s] - last * CLIP_SHIFT[1] - lists[0]["y"][i]
        wrong += bool(abs(dx) > wrong_px or abs(dy) > wrong_px)
    gaps = ident["gap"][ident["val"] == REACQUIRED]
    return len(alive), len(regained), wrong, int(gaps.max()) if len(gaps) else -1
