"""KLT_OPT_L0_LAZY_GRAD: the host's rule for a context's pyramid slots restated in plain Python, no GPU -- which builds go out lean
(wants_lean, the grouping of a batch: api_frames.hip; the plan's `lean`: l0_plan.h), which tracker launches have a lazy form (plan_track's
`lazy_capable` and `lazy`: track_plan.h; launch_pairs: api_track.hip) and who makes level-0 records on demand (ensure_level0_records and its
ten call sites).  For a sequence of operations the model predicts
  * after every build, what klt_level0_lean and klt_level0_lean_form say (the last group, as the context reports it);
  * for every call, the launches of family "gradients" (klt_timing_read): those of a build's levels >= 1 -- one merged launch per group
    of <= 16 frames, else one per level -- plus one per <= 32 slots of one size that hold a compact image and no records when a reader
    asks for them, and none otherwise.
It also holds the operation kinds, the hand-written table and the seeded generator that tests/test_gpu_lean_readers.py runs on two
contexts (one never lean, one lean) and tests/test_lean_state_rule.py holds against the conditions it was written for.

An operation is a tuple (kind, arguments ...).  Slots 0 .. 31 hold sixteen frame pairs (pair i = slots 2 i, 2 i + 1)."""
import numpy as np

from test_gpu_l0_lean import shapes_of, takes_geometry
from test_gpu_l0_lean_wave import goes_lean

MAX_BATCH = 32                   # KLT_MAX_BATCH
WORKGROUPS = 2048                # the streaming kernels' grid bound (L0S_MIN_WGS, L0W_MIN_WGS)
QUAD_MIN = 2048                  # features x pairs from which the 7x7 quad tracker runs (TRACK_QUAD7_MIN)
OPT_TRACK_VARIANT, OPT_BUILD_STREAM, OPT_TRACK_TREE_SUMS, OPT_L0_STREAM, OPT_L0_LAZY_GRAD, OPT_L0_LEAN_FORM = 11, 15, 18, 21, 22, 23
LEVELS, SS = 3, 4
BORDER = 120                     # make_tc(levels=3, ss=4): KLTUpdateTCBorder's border, windows 7 (and, kept, 9)
NSLOTS, NPAIRS = MAX_BATCH, MAX_BATCH // 2
N_BATCH, N_LONG, N_SHORT, N_SHARED = 128, 2048, 300, 700      # list lengths: 16 x 128 = 2048; one pair of 2048; below it; 3 x 700 >= 2048
TAPS = {0.1: 5, 0.2: 9}          # smooth_sigma_fact -> smoothing taps


def frame_shape():
    """(ncols, nrows): the smallest frame the production rule sends to the wide streaming kernel at 32 frames (shapes_of, tests/
    test_gpu_l0_lean.py) that leaves 16 pixels or more inside the tracking border in both directions, so that a feature list fits"""
    fits = [(nc, nr) for nc, nr, _ in shapes_of("wide") if nc - 2 * BORDER >= 16 and nr - 2 * BORDER >= 16]
    return min(fits, key=lambda s: s[0] * s[1])


NCOLS, NROWS = frame_shape()


def lean_launch(ncols, nrows, batch, stream):
    """plan_level0's `lean` (asked for) for u8 frames, three levels, subsampling 4, 5 or 9 smoothing taps: the launch of `batch` frames is a streaming kernel's"""
    return goes_lean(ncols, nrows, batch) if stream == 2 else takes_geometry("narrow", ncols, nrows, batch)


def least_lean_batch(stream=2):
    """the fewest frames of the tests' size whose launch has a lean form"""
    return min(b for b in range(1, MAX_BATCH + 1) if lean_launch(NCOLS, NROWS, b, stream))


class Slot:
    def __init__(self):
        self.nc = self.nr = 0
        self.pyr_valid = self.rec0_valid = self.l0img_valid = self.lazy_read = self.rec0_asked = False
        self.built_nc = self.built_nr = self.built_cfg = 0
        self.wanted = False          # wants_lean at its last build
        self.since = set()           # what happened to it since: "lazy_read", "asked:<kind>", "fallback"

    def form(self):
        if not self.pyr_valid:
            return "none"
        return "both" if self.rec0_valid and self.l0img_valid else "lean" if self.l0img_valid else "full"


# reader kinds: the operations that look at level 0 of built slots
READERS = ("track_plain_batch", "track_plain_single", "track_short", "track_fb", "track_guess", "track_fb_guess", "track_light", "track_w9",
           "track_variant0", "track_tree_sums", "track_affine", "quality_single", "quality_batch", "select", "select_prepared",
           "select_masked", "select_grid", "download", "shared_slot_batch")
OTHERS = ("build_all", "build_some", "build_one", "build_other_size", "swap_pairs", "retap")
KINDS = READERS + OTHERS


def pair_slots(i):
    return [2 * i, 2 * i + 1]


def slots_of(op):
    """the slots an operation reads or builds, in the order the host sees them"""
    kind = op[0]
    if kind in ("build_all", "track_plain_batch", "track_variant0"):
        return list(range(NSLOTS)) if kind == "build_all" else [s for i in range(NPAIRS) for s in pair_slots(i)]
    if kind == "build_some":
        return list(range(2 * op[1]))
    if kind in ("build_one", "build_other_size", "select", "select_prepared", "select_masked", "select_grid", "download"):
        return [op[1]]
    if kind in ("track_fb", "track_guess") and op[2]:
        return pair_slots(op[1]) + pair_slots((op[1] + 1) % NPAIRS)
    if kind == "quality_batch":
        return [s for i in range(op[1], op[1] + op[2]) for s in pair_slots(i % NPAIRS)]
    if kind == "shared_slot_batch":
        return [0, 1, 1, 2, 2, 3]
    if kind == "swap_pairs":
        return pair_slots(op[1]) + pair_slots(op[2])
    if kind == "retap":
        return []
    return pair_slots(op[1])


class Model:
    """one context's slots.  apply(op) -> {"kind", "lean", "form" (builds: the last group's; else None), "grads" (gradient launches of the
    call), "demand" (those of them that made records on demand), "forms" (what the slots read held when the call came), "groups"
    (builds: (frames, lean) per group)}; self.builds collects, per slot of every build, what the rule test asks about."""

    def __init__(self, lazy, stream=2, lean_form=1):
        self.lazy, self.stream, self.lean_form = lazy, stream, lean_form
        self.cfg_gen, self.sigma = 1, 0.1
        self.window, self.variant, self.tree_sums = 7, 4, False
        self.slots = [Slot() for _ in range(NSLOTS)]
        self.builds = []

    # ---- api_frames.hip
    def wants_lean(self, s):
        if self.lazy == 2:
            return True
        return (self.lazy == 1 and s.lazy_read and not s.rec0_asked and s.built_nc == s.nc and s.built_nr == s.nr
                and s.built_cfg == self.cfg_gen)

    def retap(self):
        """klt_set_kernels with other taps: every slot is invalid until it is built"""
        self.cfg_gen += 1
        for s in self.slots:
            s.pyr_valid = False

    def upload(self, k, nc=NCOLS, nr=NROWS):
        s = self.slots[k]
        s.nc, s.nr, s.pyr_valid = nc, nr, False

    def build(self, ids):
        sl = [self.slots[k] for k in ids]
        done, groups, grads, lean = [False] * len(sl), [], 0, False
        for i0 in range(len(sl)):
            if done[i0]:
                continue
            g = []
            for i in range(i0, len(sl)):
                if len(g) < MAX_BATCH and not done[i] and (sl[i].nc, sl[i].nr) == (sl[i0].nc, sl[i0].nr) and \
                        self.wants_lean(sl[i]) == self.wants_lean(sl[i0]):
                    g.append(sl[i])
                    done[i] = True
            want = self.wants_lean(g[0])
            lean = want and lean_launch(g[0].nc, g[0].nr, len(g), self.stream)
            grads += 1 if len(g) * (LEVELS - 1) <= MAX_BATCH else LEVELS - 1
            groups.append((len(g), lean))
            for s in g:
                self.builds.append(dict(before=s.wanted, want=want, lean=lean, since=frozenset(s.since), group=len(g), batch=len(sl),
                                        resized=s.built_nc != 0 and (s.built_nc, s.built_nr) != (s.nc, s.nr),
                                        retapped=s.built_cfg != 0 and s.built_cfg != self.cfg_gen))
                s.pyr_valid, s.rec0_valid, s.l0img_valid = True, not lean, lean
                s.lazy_read = s.rec0_asked = False
                s.built_nc, s.built_nr, s.built_cfg = s.nc, s.nr, self.cfg_gen
                s.wanted, s.since = want, set()
        form = 0 if not lean else 2 if self.lean_form == 1 and g[0].nc >= 256 and g[0].nr >= TAPS[self.sigma] else 1
        return groups, grads, lean, form

    def ensure(self, ids, asked, kind):
        """ensure_level0_records: the launches it sends out"""
        todo = []
        for k in ids:
            s = self.slots[k]
            assert s.pyr_valid, "the sequence reads slot %d, which holds no pyramids" % k
            if asked:
                s.rec0_asked = True
                s.since.add("asked:" + kind)
            if s.rec0_valid or s in todo:
                continue
            assert s.l0img_valid
            todo.append(s)
        launches, done = 0, [False] * len(todo)
        for i0 in range(len(todo)):
            if done[i0]:
                continue
            n = 0
            for i in range(i0, len(todo)):
                if n < MAX_BATCH and not done[i] and (todo[i].nc, todo[i].nr) == (todo[i0].nc, todo[i0].nr):
                    done[i], n = True, n + 1
            launches += 1
        for s in todo:
            s.rec0_valid = True
            if not asked:
                s.since.add("fallback")
        return launches

    # ---- api_track.hip
    def lazy_capable(self, n, npairs):
        return self.variant != 0 and self.window == 7 and n * npairs >= QUAD_MIN and not self.tree_sums and n > 0 and npairs > 0

    def track_plain(self, ids, n, npairs, kind):
        """launch_pairs, its records on demand and its marks, for a plain launch on `ids` (a slot may be listed more than once)"""
        capable = self.lazy_capable(n, npairs)
        launches = 0
        if not (capable and all(self.slots[k].l0img_valid for k in ids)):
            launches = self.ensure(ids, not capable, kind)
        for k in ids:
            assert self.slots[k].pyr_valid
            if capable:
                self.slots[k].lazy_read = True
                self.slots[k].since.add("lazy_read")
        return launches

    def one_by_one(self, ids, kind):
        """check_pair without a lazy form: the records of the first slot, then those of the second"""
        return sum(self.ensure([k], True, kind) for k in ids)

    def apply(self, op):
        kind, ids = op[0], slots_of(op)
        out = dict(kind=kind, lean=None, form=None, grads=0, demand=0, groups=None, forms=None)
        if kind in READERS:
            out["forms"] = [self.slots[k].form() for k in ids]
        d = 0
        if kind in ("build_all", "build_some", "build_one"):
            for k in ids:
                self.upload(k)
            out["groups"], out["grads"], out["lean"], out["form"] = self.build(ids)
        elif kind == "build_other_size":
            self.upload(ids[0], NCOLS, NROWS - 1)
            _, g1, _, _ = self.build(ids)
            self.upload(ids[0])
            out["groups"], g2, out["lean"], out["form"] = self.build(ids)
            out["grads"] = g1 + g2
        elif kind == "track_plain_batch":
            d = self.track_plain(ids, N_BATCH, NPAIRS, kind)
        elif kind == "track_plain_single":
            d = self.track_plain(ids, N_LONG, 1, kind)
        elif kind == "track_short":
            d = self.track_plain(ids, N_SHORT, 1, kind)
        elif kind == "shared_slot_batch":
            d = self.track_plain(ids, N_SHARED, 3, kind)
        elif kind in ("track_fb", "track_guess"):
            d = self.ensure(ids, True, kind) if op[2] else self.one_by_one(ids, kind)      # (batched: one launch for all)
        elif kind in ("track_fb_guess", "track_light", "quality_single"):
            d = self.one_by_one(ids, kind)
        elif kind == "track_w9":
            # the smoothing sigma is a factor times the window: a window of 9 changes the taps (by an ulp, under the factor that keeps the
            # sigma), so every slot is invalid before and after, and the operation builds all 32 itself
            self.retap()
            for k in range(NSLOTS):
                self.upload(k)
            out["groups"], grads, out["lean"], out["form"] = self.build(list(range(NSLOTS)))
            if op[2]:
                d = self.one_by_one(ids, "download")
            out["forms"] = [self.slots[k].form() for k in ids]
            self.window = 9
            d += self.track_plain(ids, N_LONG, 1, kind)
            self.window = 7
            self.retap()
            out["demand"], out["grads"] = d, d + grads
            return out
        elif kind == "track_variant0":
            self.variant = 0
            d = self.track_plain(ids, N_BATCH, NPAIRS, kind)
            self.variant = 4
        elif kind == "track_tree_sums":
            self.tree_sums = True
            d = self.track_plain(ids, N_LONG, 1, kind)
            self.tree_sums = False
        elif kind == "track_affine":
            d = self.track_plain(ids, op[2], 1, kind) + self.one_by_one(ids, kind)
        elif kind == "quality_batch":
            d = self.ensure(ids, True, kind)
        elif kind in ("select", "select_masked", "select_grid"):
            d = self.ensure(ids, True, kind)
        elif kind == "select_prepared":
            d = self.ensure(ids, True, kind) + self.ensure(ids, True, kind)         # the preparation, then the selection
        elif kind == "download":
            d = self.ensure(ids, True, kind) if op[3] == 0 else 0
            if op[3] != 0:
                assert self.slots[ids[0]].pyr_valid
        elif kind == "swap_pairs":
            out["forms"] = [self.slots[k].form() for k in ids]
            for a, b in zip(pair_slots(op[1]), pair_slots(op[2])):
                self.slots[a], self.slots[b] = self.slots[b], self.slots[a]
        elif kind == "retap":
            self.sigma = 0.2 if self.sigma == 0.1 else 0.1
            self.retap()
        else:
            raise KeyError(kind)
        if kind in READERS:
            out["demand"] = out["grads"] = d
        return out

    def run(self, ops):
        return [self.apply(op) for op in ops]


# ------------------------------------------------------------------------------------------------------------------ the fixed table
PROLOGUE = [("build_all",), ("track_plain_batch",), ("build_all",)]       # a slot's first build is full; read by the lazy tracker: lean

# every reader kind, on pair (or slot of pair) p; "download" walks its planes below
_WALK = [lambda p: ("track_plain_batch",), lambda p: ("track_plain_single", p), lambda p: ("track_short", p), lambda p: ("track_fb", p, False),
         lambda p: ("track_fb", p, True), lambda p: ("track_guess", p, False), lambda p: ("track_guess", p, True),
         lambda p: ("track_fb_guess", p), lambda p: ("track_light", p, N_SHORT), lambda p: ("track_light", p, N_LONG),
         lambda p, made=False: ("track_w9", p, made), lambda p: ("track_variant0",), lambda p: ("track_tree_sums", p), lambda p: ("track_affine", p, N_SHORT),
         lambda p: ("track_affine", p, N_LONG), lambda p: ("quality_single", p), lambda p: ("quality_batch", p, 2),
         lambda p: ("select", 2 * p), lambda p: ("select_prepared", 2 * p + 1), lambda p: ("select_masked", 2 * p),
         lambda p: ("select_grid", 2 * p, 1), lambda p: ("select_grid", 2 * p + 1, 2), lambda p: ("download", 2 * p, 0, 0),
         lambda p: ("download", 2 * p + 1, 1, 0), lambda p: ("download", 2 * p, 2, 0), lambda p: ("download", 2 * p, 0, 1),
         lambda p: ("shared_slot_batch",)]


def _relean(model, ops, ids):
    """until the slots `ids` are lean alone: a lazy tracker launch on every pair and a build of new content"""
    for _ in range(4):
        if all(model.slots[k].form() == "lean" for k in ids):
            return
        built = all(s.pyr_valid for s in model.slots)
        for op in ((("track_plain_batch",), ("build_all",)) if built else (("build_all",),)):
            model.apply(op)
            ops.append(op)
    raise AssertionError("slots %r do not go lean" % (ids,))


def fixed_table():
    """The hand-written walk: after the prologue, every reader kind once directly after a lean build of new content and once directly
    after another reader (a download of grady) has made the records of the slots it reads; then the state changes one by one."""
    m = Model(1)
    ops = list(PROLOGUE)
    m.run(ops)
    for j, make in enumerate(_WALK):
        p = (3 * j) % NPAIRS if make(0)[0] not in ("shared_slot_batch",) else 0
        op = make(p)
        ids = sorted(set(slots_of(op)))
        _relean(m, ops, ids)
        if ops[-1][0] != "build_all" and op[0] != "track_w9":       # directly after a lean build of new content
            for o in (("track_plain_batch",), ("build_all",)):
                m.apply(o)
                ops.append(o)
            assert all(m.slots[k].form() == "lean" for k in ids)
        m.apply(op)
        ops.append(op)
        # ... and again once a download has made the records: on the pair next to it (the kinds on every slot: after a build of their own)
        op2 = make((p + 1) % NPAIRS, True) if op[0] == "track_w9" else make((p + 1) % NPAIRS)
        ids2 = sorted(set(slots_of(op2)))
        _relean(m, ops, ids2)
        for k in ids2:
            o = ("download", k, 2, 0)
            m.apply(o)
            ops.append(o)
        m.apply(op2)
        ops.append(op2)
    low = least_lean_batch() // 2                            # pairs: 2 low slots are one short of the bound or at it
    ops += [("track_plain_batch",), ("build_all",),          # slots 0 .. 3, whose records the last downloads asked for, full; the rest lean
            ("swap_pairs", 0, 5), ("download", 10, 1, 0), ("swap_pairs", 10, 3), ("track_plain_single", 3), ("track_plain_single", 10),
            ("track_plain_batch",), ("build_some", low), ("track_plain_batch",), ("build_some", low + 1),      # below the bound, then above
            ("track_plain_batch",), ("build_all",),
            ("track_plain_batch",), ("build_one", 7), ("build_all",),      # a slot built alone between two batches: 31 lean, itself full
            ("track_plain_batch",), ("build_other_size", 9), ("track_plain_batch",), ("build_all",),           # a changed frame size
            ("track_plain_batch",), ("retap",), ("build_all",), ("track_plain_batch",), ("build_all",),        # changed taps
            ("select", 30), ("quality_batch", 0, 2), ("track_plain_batch",), ("build_all",),                   # a split batch: 6 full, 26 lean
            ("quality_batch", 0, 5), ("track_plain_batch",), ("build_all",),                                   # ... 10 full, 22 below the bound
            ("track_short", 2), ("shared_slot_batch",), ("track_plain_batch",), ("build_all",),
            ("download", 4, 1, 0), ("download", 4, 1, 0), ("build_other_size", 6), ("quality_batch", 2, 2), ("retap",), ("build_all",)]
    return ops


# ---------------------------------------------------------------------------------------------------------------- the seeded generator
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7]
SEQUENCE_OPS = 25


def seeded_sequence(seed, count=SEQUENCE_OPS):
    """the prologue and `count` drawn operations: builds about a third of the time (mostly of every slot), readers on drawn pairs"""
    rng = np.random.default_rng([seed, 77])
    m = Model(1)
    ops = list(PROLOGUE)
    m.run(ops)
    low = least_lean_batch() // 2
    while len(ops) < len(PROLOGUE) + count:
        r = rng.random()
        p = int(rng.integers(NPAIRS))
        if r < 0.22:
            new = [("track_plain_batch",), ("build_all",)] if rng.random() < 0.7 else [("build_all",)]
        elif r < 0.30:
            new = [("build_some", int(rng.choice([low, low + 1, 3])))]
        elif r < 0.35:
            new = [("build_one", int(rng.integers(NSLOTS)))]
        elif r < 0.39:
            new = [("build_other_size", int(rng.integers(NSLOTS)))]
        elif r < 0.43:
            new = [("retap",), ("build_all",)]
        elif r < 0.48:
            new = [("swap_pairs", p, int((p + 1 + rng.integers(NPAIRS - 1)) % NPAIRS))]
        else:
            make = _WALK[int(rng.integers(len(_WALK)))]
            new = [make(p)]
            if new[0][0] == "track_w9":
                new = [("track_w9", p, bool(rng.integers(2))), ("build_all",)]
        for op in new:
            m.apply(op)
            ops.append(op)
    return ops
