"""Device-resident sequence tracking: the call pattern of upstream KLT's example3 (select once; per frame
KLTTrackFeatures in sequentialMode, KLTReplaceLostFeatures, KLTStoreFeatureList) without a host round trip per frame.

The per-frame feature lists are the rows of ONE device-side [nFrames x nFeatures] record array (feature-buffer views,
include/klt_gpu.h klt_featbuf_view); row k-1 is the tracker's input and row k its output, replacement runs in place on
row k, and the whole table is downloaded once at the end into a KLT_FeatureTable.  Results
are bit-identical to the per-frame host API loop, which the GPU tests check.
"""
from __future__ import print_function

import contextlib

import numpy as np

from ._frames import cache_of, pixels_of
from .backend import (CROWD_DTYPE, FB_CHUNK, FEAT_DTYPE, IDENT_DTYPE, QUALITY_DTYPE, REPLACING_SOME, SELECTING_ALL, Context, context_of,
                      _FB_GUESS, _FB_TABLE, _FBC_TABLE, _FBI_TABLE, _FBQ_TABLE, _MAX_FRAMES)       # (backend.py has the table of feature-buffer ids)
from .klt import KLT_FeatureTable
from .params import (NO_POST_TRACK, equalization_for_frames, equalize_params_from_tc, fb_params_from_tc, light_params_from_tc, motion_prediction_from_tc, post_track_from_tc, reacquire_params_from_tc, remap_for_frames, remap_from_tc,
                     select_grid_from_tc, selection_mask_from_tc)
from .selectGoodFeatures import _fix_window, _slots_of

_track_dispatch_async, _post_track_async = Context.track_dispatch_async, Context.post_track_async
_OPT_SELECT_AFFINE_STATE = 4
_OPT_BUILD_STREAM = 15
_OPT_COPY_STREAMS = 20
SEQUENCE_COPY_STREAMS = 1        # copy streams a sequence call's uploads use (the default of a context, two, is for the two frames of a pair)
STAGER_WORKERS = 0                       # 0: by frame size (below); 1 / 2 / ...: that many helper threads
STAGER_THREADS_FROM_BYTES = 4 << 20      # frames of this size and above are staged by two helper threads (one core copies a 4K frame in
                                         # 0.26 ms -- longer than the GPU needs for it; tools/stage_copy_probe.py)


class _FrameStager:
    """Reads the frames and copies them into pinned staging buffers on helper threads (the copy and the frame source's decoding
    release the GIL), so that the host copy of frame k+2 -- 2 MB at 1080p, as long as the tracker of a frame runs -- is made while the
    calling thread waits for the GPU in frame k's replacement pass.  Every call into the library's device side stays on the calling
    thread.  With `workers` > 1 several frames are copied at the same time, each by one core: the iterator is advanced and the
    staging buffer taken under one lock, in frame order (so the buffers are handed out exactly as a single helper would), the copies
    run side by side, and `next()` delivers the frames in order."""

    def __init__(self, frames, buffers, shape, workers=1):
        import queue
        import threading
        self._frames, self._shape = frames, shape
        self._float = bool(buffers) and buffers[0].dtype == np.float32     # the staging buffers take float frames (colour / float images)
        self._free = queue.Queue()
        self._stop = threading.Event()
        self._pull = threading.Lock()               # advancing the iterator + taking a buffer: one frame at a time, in order
        self._cv = threading.Condition()            # results by frame index
        self._results, self._next_in, self._next_out, self._ended = {}, 0, 0, False
        for b in buffers:
            self._free.put(b)
        self._threads = [threading.Thread(target=self._run, name="klt-frame-stager-%d" % i, daemon=True) for i in range(max(1, workers))]
        for t in self._threads:
            t.start()

    def _publish(self, idx, kind, item):
        with self._cv:
            self._results[idx] = (kind, item)
            self._cv.notify_all()

    def _run(self):
        from ._abi import load_library
        from ._frames import FrameKey
        load_library().klt_host_thread_serial(1)            # (one core per frame: spread over the pool's lanes this background copy slowed the loop, profiles/README.md)
        while True:
            idx = None
            try:
                with self._pull:
                    if self._stop.is_set() or self._ended:  # closed (no further frame is pulled, no buffer written) / the source has ended
                        return
                    idx = self._next_in
                    try:
                        img = next(self._frames)
                    except StopIteration:
                        self._ended = True
                        self._publish(idx, None, None)
                        return
                    except BaseException as e:              # noqa: BLE001 -- the source failed: said at this frame's place, under the lock
                        self._ended = True                  # (another helper must not pull from the dead iterator and report the END here)
                        self._publish(idx, "error", e)
                        return
                    self._next_in = idx + 1
                    key = FrameKey(img)                     # (a Pillow image is read through its row table: no array is made of it)
                    kind = key.stage_kind()                 # ("u8" | "rgbx" | "f32", shape) of what can be written straight into a buffer
                    if kind is None and self._float and isinstance(img, np.ndarray) and img.dtype == np.float32 and img.ndim == 2:
                        kind = ("array", img.shape)
                    if kind is None or tuple(kind[1]) != tuple(self._shape) or (kind[0] == "u8") == self._float:
                        self._publish(idx, "raw", key.array())      # the calling thread deals with it (size error, or a synchronous upload)
                        continue
                    buf = self._free.get()
                    if buf is None or self._stop.is_set():
                        return
                if kind[0] == "rgbx":
                    key.float_into(buf)                     # Pillow's luma of a colour frame, straight into the pinned float buffer
                else:
                    key.copy_into(buf)
                self._publish(idx, "staged", buf)
            except BaseException as e:                      # noqa: BLE001 -- handed to the calling thread
                self._ended = True
                self._publish(self._next_in if idx is None else idx, "error", e)
                return

    def next(self):
        with self._cv:
            while self._next_out not in self._results:
                self._cv.wait()
            kind, item = self._results.pop(self._next_out)
            if kind is not None and kind != "error":
                self._next_out += 1                         # (the end and an error are final: asked again, they answer again)
            else:
                self._results[self._next_out] = (kind, item)
        if kind == "error":
            raise item
        return kind, item

    def release(self, buf):
        self._free.put(buf)

    def close(self):
        """Stops the helper threads: the stop flag is looked at before every frame and before every copy, the free queue is drained
        (so that no thread can pick up a buffer any more) and a sentinel per thread wakes one waiting for a buffer.  Returns True
        when every thread has ended -- only then may the staging buffers be handed to somebody else."""
        import queue
        self._stop.set()
        try:
            while True:
                self._free.get_nowait()
        except queue.Empty:
            pass
        for _ in self._threads:
            self._free.put(None)
        for t in self._threads:
            t.join(timeout=2.0)               # (a frame source that blocks keeps its daemon thread; it touches no buffer any more)
        return not any(t.is_alive() for t in self._threads)


def KLTTrackSequence(tc, frames, nFeatures, replace_lost=True, async_ingest=True, prefetch=True):
    """Track `nFeatures` features through `frames` (an iterable of equally sized 8-bit images) and return the
    KLT_FeatureTable: row 0 = the selected features, row k = the features after tracking frame k-1 -> k (and, with
    `replace_lost`, after replacing the lost ones on frame k: new features carry their eigenvalue in `val`, as after
    KLTReplaceLostFeatures).  tc.affineConsistencyCheck >= 0 runs the affine check on every step,
    tc.forwardBackwardCheck the forward-backward check (rejected features are lost ones: the replacement pass fills their slots).
    tc.selectionMask (zero = no feature here) holds for the first selection and every replacement; it is read once, when the call starts.
    tc.selectionGrid = (cell_width, cell_height, max_per_cell) likewise: no cell holds more than max_per_cell features after any of them.
    tc.motionPrediction = "constant_velocity": from the second step on every feature's search starts at its position plus its last
    displacement (klt_predict_cv_async on the two last rows of the table, then klt_track_guess_async: the previous list and the guesses
    never leave the device); a feature the last step lost or replaced starts at its own position.  Not together with the affine check.
    tc.trackQuality = True: the table carries `ft.quality`, a [frames][features] array of backend.QUALITY_DTYPE records -- row k measured between
    rows k - 1 and k as the tracker left them (before the replacement pass: a refilled slot is not measured), row 0 all val = 0.
    tc.motionModelCheck = "affine": one motion-model check per frame behind the tracker and in front of that frame's replacement pass, which
    refills the slots it flagged (KLT_MODEL_OUTLIER); `ft.models` holds one backend.MODEL_DTYPE record per frame, row 0 all zero.  Not
    together with the affine consistency check.
    tc.epipolarCheck = True: one epipolar check per frame in the same place (never both); the replacement pass refills the slots it flagged
    (KLT_EPIPOLAR_OUTLIER); `ft.epipolar` holds one backend.EPIPOLAR_DTYPE record per frame, row 0 all zero.
    tc.homographyCheck = True: one homography check per frame in the same place (never with either of the two); the replacement pass refills
    the slots it flagged (KLT_HOMOGRAPHY_OUTLIER); `ft.homography` holds one backend.HOMOGRAPHY_DTYPE record per frame, row 0 all zero.
    tc.crowdingCheck = True: one crowding check per frame behind the tracker and any of the checks above, in front of the quality launch and
    of that frame's replacement pass, which refills the slots it flagged (KLT_CROWDED): after every frame no two live features are within
    tc.crowding_min_distance - 1 px (None: tc.mindist) of each other.  `ft.crowd` is a [frames][features] array of backend.CROWD_DTYPE
    records -- age (the consecutive frames the slot has been tracked: the older of two colliding tracks stays), winner, val -- row k
    computed from row k - 1 and list row k, row 0 all zero.  Not together with the affine consistency check.
    tc.equalization = "clahe": every frame is equalised on the device in front of its pyramid build (tc.clahe_tiles, tc.clahe_clip_limit;
    DESIGN.md section 9l); the clip must then be of single-channel 8-bit frames the tile grid fits (ValueError).
    tc.remap = a KLT_RemapTable: every frame is remapped on the device in front of its pyramid build and of the equalisation (DESIGN.md
    section 9m); the clip must then be of single-channel 8-bit frames of the table's shape (ValueError).
    tc.reacquireLost = True: every slot of every frame gets a persistent track id, and a lost track whose corner is selected again within
    tc.reacquire_max_gap frames gets its old id back (tc.reacquire_radius, tc.reacquire_capacity,
    tc.reacquire_max_distance, tc.reacquire_ratio, tc.descriptorOrientation).  `ft.ident` is a [frames][features] array of
    backend.IDENT_DTYPE records -- id, gap (frames the track was away), distance (Hamming, of the match), val 0 no track / 1 continued /
    2 new / 3 re-acquired -- row k computed on the device from list row k as the replacement pass left it, ident row k - 1 and frame k;
    nothing is added to the host's look per frame.  The clip must be of single-channel 8-bit frames (ValueError).
    `prefetch`: the pyramids of frame k+1 are built on a second HIP stream (KLT_OPT_BUILD_STREAM) while frame k is tracked and its
    lost features are replaced -- same results, the frames then live in a ring of three slots."""
    fb_params_from_tc(tc)                # (ValueError for the forward-backward and the affine check together, before any device work)
    selection_mask_from_tc(tc)           # (TypeError for a tc.selectionMask of an unknown kind, likewise)
    grid = select_grid_from_tc(tc)       # (TypeError / ValueError for a tc.selectionGrid that is no (cell_width, cell_height, max_per_cell), likewise)
    motion_prediction_from_tc(tc)        # (ValueError for an unknown tc.motionPrediction, or one together with the affine check, likewise)
    light_params_from_tc(tc, sequence=True)      # (ValueError: tc.lightingCompensation is offered by KLTTrackFeatures alone)
    post_track_from_tc(tc)               # (ValueError for a consensus check's or tc.crowdingCheck's switch or parameters, or a check beside one, likewise)
    equalize_params_from_tc(tc)          # (ValueError for an unknown tc.equalization or parameters out of range, likewise)
    remap_from_tc(tc)                    # (TypeError for a tc.remap that is no KLT_RemapTable, likewise)
    if reacquire_params_from_tc(tc) is not None:     # (TypeError / ValueError for the switches of the track identities, likewise)
        from .describeFeatures import descriptor_mode_from_tc
        descriptor_mode_from_tc(tc)
    ctx = context_of(tc)
    with ctx.lock:                       # one KLT* call at a time per device context (backend.default_context)
        ctx.settle_deferred()
        return _track_sequence_locked(ctx, tc, frames, nFeatures, replace_lost, async_ingest, prefetch, grid)


class _RecordTable:
    """One device-side table of a sequence call: `records` feature records per frame, row k a feature-buffer view of its own.  The frames are
    consumed lazily, so the table grows in chunks of `chunk` rows (a generator of unknown length works): chunk ci is feature buffer
    base + ci * (chunk + 1), allocated with its `chunk` views -- the ids behind it -- when a row of it is first asked for.  `limit`: the call is
    refused when the table would outgrow that many ids (the feature table's); `skip_empty`: a table of rows without records is not downloaded."""

    def __init__(self, ctx, base, records, chunk=FB_CHUNK, limit=None, skip_empty=False):
        self.ctx, self.base, self.records, self.chunk, self.limit, self.skip_empty = ctx, base, records, chunk, limit, skip_empty
        self.chunks = []                     # the chunks' feature buffers

    def row(self, k):
        ci, off = divmod(k, self.chunk)
        if ci == len(self.chunks):
            chunk, records, base = self.chunk, self.records, self.base + ci * (self.chunk + 1)
            if self.limit is not None and ci * (chunk + 1) + chunk + 1 > self.limit:
                raise ValueError("sequence too long for one call")
            self.ctx.featbuf_alloc(base, chunk * records)
            for j in range(chunk):
                self.ctx.featbuf_view(base + 1 + j, base, j * records, records)
            self.chunks.append(base)
        return self.chunks[ci] + 1 + off

    def download(self, nframes, out=None):
        """the (nframes, records) array of klt_feat records (`out`, or a new one: rows nobody wrote are zero).  A chunk exists only once
        a row of it was asked for, and rows are asked for only for frames that arrived: every chunk has rows to fetch."""
        rec = np.zeros((nframes, self.records), FEAT_DTYPE) if out is None else out
        for ci, base in enumerate(self.chunks):
            lo = ci * self.chunk
            hi = min(nframes, lo + self.chunk)
            if hi > lo and (self.records or not self.skip_empty):
                self.ctx.featbuf_download_into(base, rec[lo:hi])      # rows lo .. hi-1 are contiguous in the table: no staging copy
        return rec


class _Sequence:
    """The state of one KLTTrackSequence call, made by its set-up: the frame slots, the post-track stages and their tables, the staging
    buffers and the helper threads.  The drivers below enqueue the steps, and `table` brings the result back."""

    def __init__(self, ctx, tc, frames, nFeatures, replace_lost, async_ingest, prefetch, grid):
        self.ctx, self.tc, self.frames, self.n, self.replace_lost, self.prefetch = ctx, tc, iter(frames), nFeatures, replace_lost, prefetch
        _fix_window(tc)
        cache_of(tc).keep_all_handles()     # pyramid handles somebody kept (ComputeImagePyramids, tc.pyramid_last) fetch their planes first
        ctx.configure(tc)
        self.s = list(_slots_of(tc))        # ring of three frame slots (the third is otherwise the per-frame API's selection slot)
        cache_of(tc).forget()               # this call fills the slots itself: what the per-frame API remembers of them is void
        self.ring = 3 if prefetch else 2
        first = pixels_of(next(self.frames))
        self.nrows, self.ncols = first.shape
        # tc.equalization = "clahe": every frame is equalised in front of its build (the library's side of ctx.configure); the clip must
        # be of 8-bit frames the tile grid fits (ValueError; `ingest` holds the later frames to it)
        self.equalized = bool(equalization_for_frames(tc, first).mode)
        # tc.remap: likewise every frame is remapped in front of its build; 8-bit frames of the table's shape (ValueError)
        self.remapped = remap_for_frames(tc, first) is not None
        # tc.selectionMask: one static mask for the first selection and every replacement of the clip (ValueError for another shape)
        ctx.sync_select_mask(selection_mask_from_tc(tc, self.ncols, self.nrows))
        ctx.sync_select_grid(grid)          # tc.selectionGrid, read when the call started: the first selection and every replacement
        self.affine = tc.affineConsistencyCheck >= 0
        self.fb_check = bool(fb_params_from_tc(tc).enabled) and not self.affine      # forward-backward check in every tracker step
        self.predict = motion_prediction_from_tc(tc) == "constant_velocity"          # a motion prior for every tracker step but the first
        # The tracker of frame k + 1 only READS the list that frame k's replacement completes, so it is enqueued before the host looks at
        # that replacement's outcome (klt_select_finish): the GPU has it queued while the host turns around.  In the rare case that the
        # look makes the selection rewrite the list, the tracker is enqueued once more.  Not with the affine check: it updates the
        # per-feature state in place, so its launch cannot simply be repeated.
        self.ahead = prefetch and replace_lost and not self.affine
        # the post-track stages: the same chain behind every tracker launch, each stage's records into a table of its own, laid out like the feature table
        self.stages = post_track_from_tc(tc, self.ncols, self.nrows)
        Context.set_post_track_params(ctx, self.stages)         # (as a plain function, like the two in `track`)
        self.check = self.stages.consensus[-1][0] if self.stages.consensus else None
        self.rows = _RecordTable(ctx, _FB_TABLE, nFeatures, limit=_MAX_FRAMES)
        self.quality_rows = _RecordTable(ctx, _FBQ_TABLE, nFeatures)
        self.model_rows = _RecordTable(ctx, self.check.fb_table, self.check.records) if self.check else None
        self.crowd_rows = _RecordTable(ctx, _FBC_TABLE, nFeatures, skip_empty=True)
        # tc.reacquireLost: an ident row per frame in a table of its own; the clip must be of 8-bit frames (`ingest` holds the later ones to it)
        self.reacquire = reacquire_params_from_tc(tc) if nFeatures > 0 else None
        self.ident_rows = _RecordTable(ctx, _FBI_TABLE, nFeatures, skip_empty=True)
        if self.reacquire is not None:
            from .describeFeatures import _describable_frame, descriptor_mode_from_tc
            _describable_frame(first)
            ctx.set_descriptor_params(descriptor_mode_from_tc(tc))
            ctx.set_reacquire_params(**self.reacquire)
            ctx.__dict__.pop("_ident_owner", None)     # (the context's one sequence is this call's now: KLTUpdateIdentities begins anew)
        workers = STAGER_WORKERS or (2 if first.nbytes >= STAGER_THREADS_FROM_BYTES else 1)
        # frames k+1 .. k+3 on their way, one being filled by each helper thread, one spare; uint8 buffers for 8-bit frames, float32 ones for
        # colour / float frames (the frame `img.convert("F")` would be, made by the helper threads: klt_upload_f32_async takes it from there)
        self.stage_key = ((self.nrows, self.ncols), self.ring + 2 + workers, first.dtype)
        stage = ctx.staging(*self.stage_key) if async_ingest and first.dtype in (np.uint8, np.float32) else None
        self.in_flight, self.stager, self.k = [], None, 0       # staging buffers whose copy may still be running; the last frame whose step was enqueued
        self.ingest(self.s[0], first, 0)
        ctx.build_pyramids(self.s[0], sync=False)
        # the initial selection follows KLTSelectGoodFeatures: the smoothed level-0 image when tc.smoothBeforeSelecting, the raw
        # frame otherwise (selectGoodFeatures.py:183-197) -- level 0 of the pyramid is always smoothed
        ctx.select_async(self.s[0], SELECTING_ALL, bool(tc.smoothBeforeSelecting), self.rows.row(0), nFeatures)
        if self.reacquire is not None:
            ctx.reacquire_begin_async(self.s[0], self.rows.row(0), self.ident_rows.row(0), nFeatures)
        self.state = ctx.take_affine_state() if self.affine else None
        if self.affine:
            ctx.affine_alloc(self.state, nFeatures)
        if stage is not None:
            self.stager = _FrameStager(self.frames, stage, (self.nrows, self.ncols), workers=workers)

    def ingest(self, slot, img, k, staged=False, wait=True):
        for on, setting in ((self.equalized, "tc.equalization = 'clahe'"), (self.remapped, "tc.remap")):
            if on and (img.dtype != np.uint8 or img.ndim != 2):
                raise ValueError("{0} takes single-channel 8-bit frames; frame {1} of the clip is not one".format(setting, k))
        if self.reacquire is not None and k > 0:
            from .describeFeatures import _describable_frame
            _describable_frame(img)
        if img.shape != (self.nrows, self.ncols):
            from .error import KLTError
            KLTError("(KLTTrackSequence) Size of incoming image ({0} by {1}) is different from size of previous image "
                     "({2} by {3})".format(img.shape[1], img.shape[0], self.ncols, self.nrows))
        if staged:
            if wait:
                self.ctx.upload_wait()      # the previous frame's copy has finished (kernels keep running): its buffer goes back
                while self.in_flight:
                    self.stager.release(self.in_flight.pop()[1])
            self.ctx.upload_async(slot, img)
            self.in_flight.append((k, img))
        else:
            self.ctx.upload(slot, img)

    def landed(self, k):
        """frame k's selection has completed, so its pyramid was built, so its copy has left the staging buffer: the buffer goes back
        (no host wait for the copy streams -- klt_upload_wait costs the host the rest of the copy)"""
        while self.in_flight and self.in_flight[0][0] <= k:
            self.stager.release(self.in_flight.pop(0)[1])

    def next_frame(self):                    # ("staged", pinned buffer) | ("raw", array) | None at the end
        if self.stager is not None:
            item = self.stager.next()
            return item if item[0] is not None else None
        img = next(self.frames, None)
        return None if img is None else ("raw", pixels_of(img))

    def stage_frame(self, k, item):          # upload + pyramid build of frame k (enqueued only)
        self.ingest(self.s[k % self.ring], item[1], k, staged=item[0] == "staged")
        self.build(k)

    def send(self, j):                       # frame j leaves for its slot, if there is one (no wait for the copy before it)
        item = self.next_frame()
        if item is not None:
            self.ingest(self.s[j % self.ring], item[1], j, staged=item[0] == "staged", wait=False)
        return item is not None

    def build(self, j):
        ctx, slot = self.ctx, self.s[j % self.ring]
        ctx.build_pyramids(slot, sync=False)
        if self.replace_lost and self.prefetch:      # ... and the list-independent half of its replacement pass, on the same stream
            ctx.select_prepare(slot)

    def track(self, j):
        """frame j - 1 -> j: row j - 1 of the table in, row j out; behind the tracker -- wherever it goes, a repeated one included -- the
        post-track stages, in front of frame j's replacement pass.  (The two Context methods are called as plain functions: what stands
        in for a context in the tests has the entry points alone.)"""
        ctx, n, row = self.ctx, self.n, self.rows.row
        cur, prev = self.s[j % self.ring], self.s[(j - 1) % self.ring]
        fb_guess = None
        if self.predict and j >= 2:          # guesses from rows j - 2 and j - 1, on the same stream in front of the tracker that reads them
            ctx.predict_cv_async(row(j - 2), row(j - 1), _FB_GUESS, n)
            fb_guess = _FB_GUESS
        fb_in, fb_out = row(j - 1), row(j)
        _track_dispatch_async(ctx, prev, cur, fb_in, fb_out, n, self.state, self.fb_check, fb_guess)
        if self.stages != NO_POST_TRACK:
            self.j = j
            _post_track_async(ctx, self.stages, prev, cur, fb_in, fb_out, n, self)

    def identify(self, k):
        """tc.reacquireLost: the identity step of frame k, enqueued once list row k is final -- behind the post-track chain, or behind the
        replacement pass's last launch (the host has looked: klt_select_finish), on the stream both run on -- and before frame k's slot
        is given to a later frame.  It reads row k and never writes it: the tracker of step k + 1, repeated or not, is unaffected."""
        if self.reacquire is not None:
            self.ctx.reacquire_step_async(self.s[k % self.ring], self.rows.row(k), self.ident_rows.row(k - 1), self.ident_rows.row(k), self.n)

    # Context.post_track_async's `targets` for step `j`: row j of each stage's table (a chunk of a table is allocated when its stage first
    # asks for a row of it); the crowding check reads row j - 1 of its own table (row 0: no ages yet)
    model = property(lambda q: q.model_rows.row(q.j))
    crowd_prev = property(lambda q: q.crowd_rows.row(q.j - 1) if q.j >= 2 else -1)
    crowd = property(lambda q: q.crowd_rows.row(q.j))
    quality = property(lambda q: q.quality_rows.row(q.j))

    def open(self, stack):
        """Sets the options of the call; `stack` (an ExitStack) undoes them when it closes, and ends what the call started, in the order
        written here -- every step on its own: a failing one must not skip the rest (the options live on the shared default context)."""
        ctx = self.ctx
        steps = [ctx.select_finish, self.close_stager, lambda: ctx.set_option(_OPT_COPY_STREAMS, 2)]      # (a look: only pending after an exception)
        if self.prefetch:
            steps.append(lambda: ctx.set_option(_OPT_BUILD_STREAM, 0))
        if self.affine:
            steps += [lambda: ctx.set_option(_OPT_SELECT_AFFINE_STATE, -1), lambda: ctx.release_affine_state(self.state)]
        for step in reversed(steps):                                       # (an ExitStack runs what it was given last first)
            stack.callback(step)
        if self.affine:
            ctx.set_option(_OPT_SELECT_AFFINE_STATE, self.state)
        if self.prefetch:
            ctx.set_option(_OPT_BUILD_STREAM, 1)
        # one new frame per step: all uploads on ONE copy stream (the default, two, is for the two frames of a pair; with two, the look at
        # every other frame's selection waits twice as long -- 0.280 against 0.307 ms per 4K frame, profiles/README.md round 6)
        ctx.set_option(_OPT_COPY_STREAMS, SEQUENCE_COPY_STREAMS)

    def close_stager(self):
        if self.stager is not None and not self.stager.close():
            # the helper thread is still inside the caller's frame source: it may yet write one buffer of this set, so the
            # next call must not get the same pinned memory (a fresh set is allocated instead)
            self.ctx.staging_forget(*self.stage_key)

    def table(self):
        """the KLT_FeatureTable of the frames that arrived: one download per chunk and table, straight into the arrays handed out"""
        nframes, stages = self.k + 1, self.stages
        ft = KLT_FeatureTable(nframes, self.n, _fill=False)
        self.rows.download(nframes, ft.rec)
        ft.rec["aux"] = 0
        if stages.quality:
            ft.quality = self.quality_rows.download(nframes).view(QUALITY_DTYPE)
            ft.quality[0] = 0                                        # nothing was tracked into the first frame
        if stages.crowd is not None:
            ft.crowd = self.crowd_rows.download(nframes).view(CROWD_DTYPE)
            ft.crowd[0] = 0                                          # nothing was tracked into the first frame
        if self.reacquire is not None:
            ft.ident = self.ident_rows.download(nframes).view(IDENT_DTYPE)
        for check, _ in stages.consensus:
            records = self.model_rows.download(nframes).view(check.dtype).reshape(nframes)
            if self.n == 0:
                records[:] = np.zeros(1, check.dtype)[0]             # (no list, no launch: nothing was written)
            records[0] = np.zeros(1, check.dtype)[0]                 # nothing was tracked into the first frame
            setattr(ft, check.ft, records)                           # ft.models, ft.epipolar or ft.homography
        if self.tc.sequentialMode:
            # leave the context as the per-frame API would: the last frame's pyramids are "frame 1" of the next call
            from .trackFeatures import _pyramid_handles
            tc, s = self.tc, self.s
            last = s[(nframes - 1) % self.ring]
            if last != s[0]:
                self.ctx.swap_slots(s[0], last)
            tc.pyramid_last, tc.pyramid_last_gradx, tc.pyramid_last_grady = _pyramid_handles(tc, self.ctx, s[0], self.ncols, self.nrows)
        return ft


def _drive_ahead(q):
    """The steps of a call that replaces lost features and prefetches: every tracker is enqueued before the host looks at the replacement
    in front of it (_Sequence.ahead), and frames are SENT two steps before their pyramid is built: frame k + 3 leaves for the slot of
    frame k (its other raw buffer) at the end of step k, while the tracker k -> k + 1 still reads that slot's pyramids.  Sent one step
    ahead, a 4K frame's 155 us copy and its build sit behind each other in front of the tracker that needs them (0.329 instead of
    0.277 ms per frame, profiles/README.md)."""
    ctx, s, ring, row, n = q.ctx, q.s, q.ring, q.rows.row, q.n
    have = 0                                 # frames sent so far beyond frame 0: 1 .. have
    for j in (1, 2):
        if have == j - 1 and q.send(j):      # (a source that has ended is not asked again: the helper thread says so only once)
            have = j
    if have >= 1:
        q.build(1)
        q.track(1)
    if have == 2 and q.send(3):              # into frame 0's slot, which only the tracker just enqueued still reads
        have = 3
    while q.k + 1 <= have:
        q.k = k = q.k + 1
        ctx.select_begin(s[k % ring], REPLACING_SOME, True, row(k), n)
        if k + 1 <= have:
            q.build(k + 1)
            q.track(k + 1)
        if ctx.select_finish() and k + 1 <= have:
            q.track(k + 1)
        q.identify(k)                        # (row k is final; before frame k + 3 is sent into this frame's slot)
        if q.stager is not None:
            q.landed(k)
        # (after the look: a repeated tracker needs slot k's pyramids valid.  Putting the send off to behind the NEXT selection's
        # launches -- so that the host is back at them sooner -- measured slower, 0.360 against 0.335 ms per 4K frame, 0.168 against
        # 0.153 at 1080p: the copy's head start is worth more than the host's 25 us)
        if have == k + 2 and q.send(k + 3):
            have = k + 3


def _drive_plain(q):
    """The steps of every other call: tracker, replacement pass up to the host's look, the next frame's upload and build in between (`prefetch`) or behind."""
    nxt = q.next_frame()
    if nxt is not None:
        q.stage_frame(1, nxt)
    while nxt is not None:
        q.k = k = q.k + 1
        nxt = q.next_frame()
        q.track(k)
        if q.replace_lost:                   # the chain first: tracker, then the replacement pass up to the host's look at it
            q.ctx.select_begin(q.s[k % q.ring], REPLACING_SOME, True, q.rows.row(k), q.n)
        if nxt is not None and q.prefetch:
            q.stage_frame(k + 1, nxt)        # the next frame's upload, build and scores: enqueued while the GPU works on the above
        if q.replace_lost:
            q.ctx.select_finish()
        q.identify(k)
        if nxt is not None and not q.prefetch:
            q.stage_frame(k + 1, nxt)


def _track_sequence_locked(ctx, tc, frames, nFeatures, replace_lost, async_ingest, prefetch, grid=None):
    q = _Sequence(ctx, tc, frames, nFeatures, replace_lost, async_ingest, prefetch, grid)
    with contextlib.ExitStack() as stack:
        q.open(stack)
        (_drive_ahead if q.ahead else _drive_plain)(q)
    return q.table()
