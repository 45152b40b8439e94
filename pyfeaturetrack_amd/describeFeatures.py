"""Not in the reference: binary descriptors of a feature list and their Hamming matcher (include/klt_gpu.h, "descriptors"; DESIGN.md
section 9n).  KLTDescribeFeatures gives every feature a 256-bit descriptor of the frame the tracker sees, KLTMatchDescriptors finds each
query's nearest and second-nearest descriptor in a train set.  Both run on the device (describe_kernels.hip, match_kernels.hip); both rules
are integer-only, and tests/describe_expected.py restates them in numpy."""
import numbers

import numpy as np

from .backend import DESCRIPTOR_DTYPE, FEAT_DTYPE, MATCH_DTYPE, context_of

# klt_match.val
KLT_MATCH_NOT_DESCRIBED, KLT_MATCHED, KLT_MATCH_NO_CANDIDATE, KLT_MATCH_TOO_FAR, KLT_MATCH_AMBIGUOUS, KLT_MATCH_NOT_MUTUAL = 0, 1, 2, 3, 4, 5


class KLT_DescriptorList:
    """A thin holder of the descriptor records of a feature list (`records`, DESCRIPTOR_DTYPE, one per feature in list order):
    .bits an (n, 32) uint8 view of the 256 bits, .val 1 described / 0 not, .orientation the bin 0 .. 31 (0 for upright descriptors),
    .x / .y the pixel the descriptor is centred on.  Indexing with a slice, a mask or an index array gives a list of those records."""

    def __init__(self, records):
        self.records = np.ascontiguousarray(records, DESCRIPTOR_DTYPE)

    def __len__(self):
        return len(self.records)

    def __getitem__(self, which):
        picked = self.records[which]
        return KLT_DescriptorList(picked.reshape(-1) if isinstance(picked, np.ndarray) else np.array([picked], DESCRIPTOR_DTYPE))

    bits = property(lambda self: self.records["bits"].view(np.uint8).reshape(len(self.records), 32))
    val = property(lambda self: self.records["val"])
    orientation = property(lambda self: self.records["orientation"])
    x = property(lambda self: self.records["cx"])
    y = property(lambda self: self.records["cy"])


def _records_of(what, name):
    if isinstance(what, KLT_DescriptorList):
        return what.records
    if isinstance(what, np.ndarray) and what.dtype == DESCRIPTOR_DTYPE and what.ndim == 1:
        return np.ascontiguousarray(what)
    raise TypeError("{0} must be a KLT_DescriptorList (KLTDescribeFeatures) or an array of descriptor records".format(name))


def descriptor_mode_from_tc(tc):
    """tc.descriptorOrientation (False, the default: upright, mode 1; True: steered, mode 2), read with a default"""
    on = getattr(tc, "descriptorOrientation", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("tc.descriptorOrientation must be True or False (got {0!r})".format(on))
    return 2 if on else 1


def _describable_frame(img):
    from .params import _frame_class
    ok, _, what = _frame_class(img)
    if not ok:
        raise ValueError("descriptors take single-channel 8-bit frames (a 2-D uint8 array or a Pillow image of mode 'L'), not {0}".format(what))


def KLTDescribeFeatures(tc, img, featurelist):
    """A KLT_DescriptorList: the 256-bit descriptor of every feature of `featurelist` (a feature list, or an array of klt_feat records)
    on `img` as the tracker sees it -- remapped under tc.remap, then equalised under tc.equalization, where those are on.  A lost
    feature (val < 0) and a position outside the frame give an undescribed record (val 0, all zero).  tc.descriptorOrientation chooses
    upright or steered descriptors.  A frame that one of the tracking context's slots already holds is not uploaded again.  ValueError
    -- before any device work -- for float and colour frames."""
    from ._frames import FrameKey, cache_of, ingest_tag, pixels_of, settle_frames
    from .params import equalization_for_frames, remap_for_frames
    from .selectGoodFeatures import _slots_of, features_to_array
    _describable_frame(img)
    mode = descriptor_mode_from_tc(tc)
    equalization_for_frames(tc, img)                    # (ValueError for a frame the tile grid does not fit)
    remap_for_frames(tc, img)                           # (TypeError / ValueError for tc.remap)
    if isinstance(featurelist, np.ndarray):
        if featurelist.dtype != FEAT_DTYPE or featurelist.ndim != 1:
            raise TypeError("a feature array must be a 1-D array of klt_feat records")
        records = np.ascontiguousarray(featurelist)
    else:
        records = features_to_array(featurelist)
    ctx = context_of(tc)
    with ctx.lock:
        ctx.settle_deferred()
        if cache_of(tc).handles and not ctx.configured_for(tc):
            cache_of(tc).keep_all_handles()             # new parameters void every pyramid of the context: kept handles fetch theirs first
        ctx.configure(tc)                               # (tc.equalization and tc.remap reach the library here)
        slots = _slots_of(tc)
        slot = cache_of(tc).find(FrameKey(img, ingest_tag(tc)), slots[:2], ctx)
        if slot is None:
            slot = slots[2]                             # the selection's own slot: neither frame of the pair is disturbed
            ctx.upload(slot, pixels_of(img))
        ctx.set_descriptor_params(mode)
        out = ctx.describe(slot, records)
        settle_frames(ctx)
    return KLT_DescriptorList(out)


def match_params(max_distance=64, ratio=(4, 5), cross_check=True, radius=None):
    """the five integers of klt_match_params from KLTMatchDescriptors' arguments; TypeError / ValueError for anything the library would
    refuse"""
    def integer(v, name):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
            raise TypeError("{0} must be an integer (got {1!r})".format(name, v))
        return int(v)
    max_distance = integer(max_distance, "max_distance")
    if not 0 <= max_distance <= 256:
        raise ValueError("max_distance must lie in 0 .. 256 (got {0})".format(max_distance))
    if ratio is None:
        num, den = 0, 1
    else:
        try:
            num, den = ratio
        except (TypeError, ValueError):
            raise TypeError("ratio must be None or a pair of integers (numerator, denominator), got {0!r}".format(ratio)) from None
        num, den = integer(num, "ratio[0]"), integer(den, "ratio[1]")
        if not 0 < num <= den <= 65535:
            raise ValueError("ratio must satisfy 0 < numerator <= denominator <= 65535 (got {0} / {1})".format(num, den))
    if not isinstance(cross_check, (bool, np.bool_)):
        raise TypeError("cross_check must be True or False (got {0!r})".format(cross_check))
    radius = 0 if radius is None else integer(radius, "radius")
    if radius < 0 or radius > 2 ** 31 - 1:
        raise ValueError("radius must be None or an integer in 0 .. 2^31 - 1 (got {0})".format(radius))
    return dict(max_distance=max_distance, ratio_num=num, ratio_den=den, cross_check=int(bool(cross_check)), radius=radius)


def KLTMatchDescriptors(tc, query, train, max_distance=64, ratio=(4, 5), cross_check=True, radius=None):
    """The klt_match records (a structured array: train, distance, second, val), one per query descriptor: `train` the nearest train
    descriptor by Hamming distance (ties to the lowest index; -1: none), `distance` to it, `second` the distance to the second nearest
    (257: none).  val: KLT_MATCHED (1), or why not -- 0 the query is not described, 2 no candidate, 3 distance > max_distance, 4 the ratio
    test (`ratio` = (num, den): matched only if distance * den < second * num; None: off), 5 the cross-check (the train descriptor's own
    nearest query is another).  radius: only train descriptors within `radius` pixels of the query on both axes are candidates (None or 0:
    no gate).  Argument errors are raised before the device is touched."""
    q, t = _records_of(query, "query"), _records_of(train, "train")
    params = match_params(max_distance, ratio, cross_check, radius)
    ctx = context_of(tc)
    with ctx.lock:
        ctx.settle_deferred()
        ctx.set_match_params(**params)
        return ctx.match(q, t)


__all__ = ["KLT_DescriptorList", "KLTDescribeFeatures", "KLTMatchDescriptors", "KLT_MATCH_NOT_DESCRIBED", "KLT_MATCHED",
           "KLT_MATCH_NO_CANDIDATE", "KLT_MATCH_TOO_FAR", "KLT_MATCH_AMBIGUOUS", "KLT_MATCH_NOT_MUTUAL", "DESCRIPTOR_DTYPE", "MATCH_DTYPE"]
