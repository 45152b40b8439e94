"""Not in the reference: persistent track identities for the reference's own loop KLTTrackFeatures + KLTReplaceLostFeatures
(include/klt_gpu.h, "track identities").  KLTUpdateIdentities(tc, img, featurelist), called once per frame with
the list as the loop left it, returns one ident record per slot: the id the slot's track carries, and -- for a newly selected feature
that matches what a lost track left behind -- the old id again.  The previous ident row, the previous descriptors and the bank of lost
tracks stay on the device (reacquire_kernels.hip); tests/reacquire_expected.py restates the rule in numpy.  KLTTrackSequence does the
same for a whole clip under tc.reacquireLost."""
import numpy as np

from .backend import FEAT_DTYPE, IDENT_DTYPE, _FB_API_IDENT, _FB_API_IDENT_IN, context_of

# klt_ident.val
KLT_IDENT_NONE, KLT_IDENT_CONTINUED, KLT_IDENT_NEW, KLT_IDENT_REACQUIRED = 0, 1, 2, 3


def KLTResetIdentities(tc):
    """The next KLTUpdateIdentities(tc, ...) begins a new sequence: ids start at 0 again and the bank of lost tracks is emptied."""
    tc.__dict__.pop("_klt_ident", None)


def KLTUpdateIdentities(tc, img, featurelist):
    """The ident records (a structured array: id, gap, distance, val) of `featurelist` (a feature list, or an array of klt_feat records)
    on `img`, the frame the list lives in.  The first call, or the first after KLTResetIdentities(tc), numbers the live features
    0 .. n - 1 by slot; every later call takes the list of the next frame -- after KLTTrackFeatures and KLTReplaceLostFeatures -- and
    gives a tracked slot (val 0) the id it had (val KLT_IDENT_CONTINUED), a newly selected one (val > 0) either the id of the lost track
    it matches (KLT_IDENT_REACQUIRED, `gap` = the frames the track was away, `distance` the Hamming distance) or the next new id
    (KLT_IDENT_NEW), and a lost one id -1.  The switches are tc.reacquire_radius, tc.reacquire_max_gap, tc.reacquire_capacity,
    tc.reacquire_max_distance, tc.reacquire_ratio and tc.descriptorOrientation, read when the sequence begins; tc.reacquireLost itself
    is KLTTrackSequence's switch and is not asked here.  The list must keep its length.  ValueError -- before any device work -- for
    float and colour frames."""
    from ._frames import FrameKey, cache_of, ingest_tag, pixels_of, settle_frames
    from .describeFeatures import _describable_frame, descriptor_mode_from_tc
    from .params import equalization_for_frames, reacquire_params_from_tc, remap_for_frames
    from .selectGoodFeatures import _slots_of, features_to_array
    _describable_frame(img)
    mode = descriptor_mode_from_tc(tc)
    params = reacquire_params_from_tc(_SwitchedOn(tc))
    equalization_for_frames(tc, img)                    # (ValueError for a frame the tile grid does not fit)
    remap_for_frames(tc, img)                           # (TypeError / ValueError for tc.remap)
    if isinstance(featurelist, np.ndarray):
        if featurelist.dtype != FEAT_DTYPE or featurelist.ndim != 1:
            raise TypeError("a feature array must be a 1-D array of klt_feat records")
        records = np.ascontiguousarray(featurelist)
    else:
        records = features_to_array(featurelist)
    n = len(records)
    if n < 1:
        raise ValueError("track identities take at least one feature")
    ctx = context_of(tc)
    with ctx.lock:
        ctx.settle_deferred()
        state = tc.__dict__.get("_klt_ident")
        # the library keeps ONE sequence per device context: another tracking context's, or a KLTTrackSequence call's, ends this one
        begin = state is None or ctx.__dict__.get("_ident_owner") is not state
        if not begin and state["n"] != n:
            raise ValueError("the feature list has {0} features; the sequence began with {1} (KLTResetIdentities starts a new one)".format(n, state["n"]))
        if cache_of(tc).handles and not ctx.configured_for(tc):
            cache_of(tc).keep_all_handles()             # new parameters void every pyramid of the context: kept handles fetch theirs first
        ctx.configure(tc)                               # (tc.equalization and tc.remap reach the library here)
        slots = _slots_of(tc)
        slot = cache_of(tc).find(FrameKey(img, ingest_tag(tc)), slots[:2], ctx)
        if slot is None:
            slot = slots[2]                             # the selection's own slot: neither frame of the pair is disturbed
            ctx.upload(slot, pixels_of(img))
        ctx.featbuf_upload(_FB_API_IDENT_IN, records)
        if begin:
            ctx.set_descriptor_params(mode)
            ctx.set_reacquire_params(**params)
            ctx.reacquire_begin_async(slot, _FB_API_IDENT_IN, _FB_API_IDENT[0], n)
            state = tc.__dict__["_klt_ident"] = ctx.__dict__["_ident_owner"] = {"n": n, "row": 0}
        else:
            prev = state["row"]
            ctx.reacquire_step_async(slot, _FB_API_IDENT_IN, _FB_API_IDENT[prev], _FB_API_IDENT[1 - prev], n)
            state["row"] = 1 - prev
        out = ctx.ident_download(_FB_API_IDENT[state["row"]], n)
        settle_frames(ctx)
    return out


class _SwitchedOn:
    """a tracking context's reacquire_* switches with reacquireLost read as True"""

    def __init__(self, tc):
        self._tc = tc

    def __getattr__(self, name):
        if name == "reacquireLost":
            return True
        return getattr(self._tc, name)


__all__ = ["KLTUpdateIdentities", "KLTResetIdentities", "KLT_IDENT_NONE", "KLT_IDENT_CONTINUED", "KLT_IDENT_NEW", "KLT_IDENT_REACQUIRED",
           "IDENT_DTYPE"]
