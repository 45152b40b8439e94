/*
 * klt_gpu.h -- C ABI of libkltgpu.so, the MI355X (gfx950) backend for the PyFeatureTrack KLT
 * hot path: pyramid build -> min-eigenvalue corner selection -> per-feature Newton tracking.
 *
 * The reference (TimSC/PyFeatureTrack) has no FFI of its own; its only native boundary is the
 * Cython `def` layer (setup.py:8-9).  Each entry point below names the reference interface it
 * replaces (file:line relative to the reference root).  Host code stays Python and binds this
 * header with ctypes (pyfeaturetrack_amd/_abi.py; INTEGRATION.md shows the stub a reference
 * maintainer would add).
 *
 * Conventions
 *   - plain C types only; no torch / HIP types cross the boundary;
 *   - every function returns 0 on success or a negative klt_status (klt_timing_read: the entry count; klt_slot_state: the
 *     state bits; klt_select_finish: also 1, "done, and the list was rewritten on the way" -- see there); the message is available
 *     from klt_last_error(); nothing exits the process or throws across the ABI
 *     (the reference's KLTError prints and calls exit(1), error.py:12-14);
 *   - per-feature failures are data (klt_feat.val < 0, klt.py:23-29), not errors;
 *   - host buffers are caller-owned and only borrowed for the duration of the call;
 *   - device buffers are owned by the context: frames live in numbered *slots* (u8/f32 image +
 *     the three pyramids), feature lists in numbered *feature buffers*;
 *   - a context owns one HIP stream; *_async entry points only enqueue, everything else has
 *     completed on return.  One context per host thread / device; no shared mutable globals;
 *   - there is NO CPU path: klt_create fails if the device cannot be opened.
 */
#ifndef KLT_GPU_H
#define KLT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KLT_ABI_VERSION 11        /* (unchanged by the forward-backward entry points, by the selection mask and by the motion prior:
                                   * klt_set_fb_params / klt_track_fb* / klt_set_select_mask* / klt_track_guess* / klt_track_fb_guess_async /
                                   * klt_predict_cv_async / klt_set_light_params / klt_track_light_path / klt_set_select_grid / klt_select_grid_path / klt_track_quality* / klt_set_model_params / klt_motion_check* / klt_motion_model_affine / klt_set_epipolar_params / klt_epipolar_check* / klt_epipolar_matrix / klt_set_homography_params / klt_homography_check* / klt_homography_matrix / klt_set_crowd_params / klt_crowd_check* / klt_set_equalize_params / klt_equalize_u8 / klt_download_equalized_u8 / klt_equalize_path / klt_set_remap / klt_remap_u8 / klt_download_remapped_u8 / klt_remap_path / klt_set_descriptor_params / klt_describe* / klt_set_match_params / klt_match* / klt_match_path are purely additive, no
                                   * existing struct or signature moved; klt_params stays as it is; nor by klt_level0_path,
                                   * klt_select_score_path, klt_select_pick_path and klt_download_prepared_keys, read-only diagnostic
                                   * entries) */
#define KLT_MAX_KERNEL_WIDTH 71   /* convolve.py:28 */
#define KLT_MAX_LEVELS 8

typedef enum {
    KLT_OK = 0,
    KLT_ERR_ARG = -1,        /* bad argument / unsupported parameter combination */
    KLT_ERR_DEVICE = -2,     /* HIP runtime error */
    KLT_ERR_STATE = -3,      /* call order (e.g. tracking a slot whose pyramids were never built) */
    KLT_ERR_NOMEM = -4,      /* a device or pinned-host allocation could not be had (klt_last_error names the size asked for); nothing is left
                              * half-allocated and no stale error is left with the HIP runtime: free something and repeat the call */
    KLT_ERR_TIMEOUT = -5     /* a host-side wait for a collective gave up (klt_comm_set_timeout): a peer is gone or stuck */
} klt_status;

/* feature status codes, klt.py:23-29 (kltState) */
enum { KLT_TRACKED = 0, KLT_NOT_FOUND = -1, KLT_SMALL_DET = -2, KLT_MAX_ITERATIONS = -3,
       KLT_OOB = -4, KLT_LARGE_RESIDUE = -5,
       KLT_FB_INCONSISTENT = -6, /* not in the reference: rejected by the forward-backward check (klt_track_fb_async); lost, like every negative val */
       KLT_MODEL_OUTLIER = -7,   /* not in the reference: off the frame pair's dominant affine motion (klt_motion_check_async); lost likewise */
       KLT_EPIPOLAR_OUTLIER = -8, /* not in the reference: off the frame pair's fundamental matrix (klt_epipolar_check_async); lost likewise */
       KLT_HOMOGRAPHY_OUTLIER = -9, /* not in the reference: off the frame pair's homography (klt_homography_check_async); lost likewise */
       KLT_CROWDED = -10          /* not in the reference: drifted within min_distance of an older track (klt_crowd_check_async); lost likewise */ };

/* selection modes, selectGoodFeatures.py:11-13 */
enum { KLT_SELECTING_ALL = 1, KLT_REPLACING_SOME = 2 };

/* 16-byte feature record; replaces the KLT_Feature attribute bag (klt.py:249-263).
 * x, y hold the reference's Python floats (integers after selection, f32-valued after tracking,
 * -1 when lost); val is the status / int(eigenvalue). */
typedef struct { float x, y; int32_t val; int32_t aux; } klt_feat;

/* POD mirror of KLT_TrackingContext (klt.py:45-73) plus the values the reference derives from it.
 * borderx/bordery are Python floats in the reference (e.g. 30.0, klt.py:186-189). */
typedef struct {
    int32_t mindist, window_width, window_height;
    int32_t smoothBeforeSelecting, retainTrackers, nSkippedPixels;
    int32_t max_iterations, nPyramidLevels, subsampling, use_max_residue;
    float   min_determinant, min_displacement, step_factor, max_residue;
    double  min_eigenvalue;
    double  grad_sigma, smooth_sigma, pyramid_sigma;
    double  borderx, bordery;
} klt_params;

typedef struct klt_ctx klt_ctx;

/* ---- lifetime ------------------------------------------------------------------------------ */
int         klt_abi_version(void);
int         klt_device_count(void);
int         klt_create(int device, klt_ctx **out);          /* replaces KLT_TrackingContext() device state, klt.py:43-81 */
void        klt_destroy(klt_ctx *ctx);
const char *klt_last_error(klt_ctx *ctx);                   /* ctx may be NULL: error of the last failed klt_create */
int         klt_sync(klt_ctx *ctx);                         /* wait for everything enqueued on the context's stream */
void       *klt_stream_handle(klt_ctx *ctx);                /* the context's hipStream_t, for callers that order RCCL collectives after it */

/* ---- options ------------------------------------------------------------------------------ */
#define KLT_OPT_FUSED_KERNELS 1   /* 1 (default): LDS-tiled fused pyramid kernels; 0: generic two-pass kernels (any tap count) */
/* affine state (klt_affine_alloc id, or -1) whose records klt_select* resets for every slot it fills
 * (selectGoodFeatures.py:120-128 clears the aff_* fields of a newly placed feature) */
#define KLT_OPT_SELECT_AFFINE_STATE 4
/* 1 (default): klt_select* only considers the highest-scoring candidates (histogram threshold keeping about 64 per
 * requested feature) and repeats with every candidate if they run out before the list is full; 0: always every candidate. */
#define KLT_OPT_TOPK_PREFILTER 5
/* 1 (default): minimum-distance enforcement as parallel passes over all candidates (a candidate is accepted once every
 * higher-ranked neighbour is rejected; same result as the walk); 0: sort all candidates and walk them in order.
 * Either way klt_select_async synchronises once internally (it reads back whether the list was filled / settled). */
#define KLT_OPT_SELECT_PARALLEL_NMS 8
#define KLT_OPT_SAT_VARIANT 10           /* summed-area tables: 1 (default) step-synchronous wavefront pipelines (frames with ncols % 4 == 0), 0 barrier-coupled kernels */
#define KLT_OPT_TRACK_VARIANT 11         /* 4 (default): quad-load tracker kernels (7x7: four features per wavefront; 15x15: one 16-byte load per lane and image); 0: plain one-feature-per-wavefront kernel for every window (same records; process-wide) */
#define KLT_OPT_FUSED_HREDUCE 12         /* 1 (default): the level-0 kernel also runs the horizontal pass of the first pyramid reduction (subsampling 4); 0: separate reduction kernel */
#define KLT_OPT_TRACK_XCD_ORDER 13        /* 1 (default): features are handed to the tracker sorted by row, one band of the image per XCD (single-pair and batched launches; the order is refreshed every 64 launches); 0: list order */
/* 1: pyramid builds are enqueued on a second HIP stream of the context (a second hardware queue), behind everything enqueued on
 * the main stream so far; trackers / selections / uploads that touch a slot wait (on the device) for the build that fills it.
 * A sequence can then enqueue the build of frame t+1 BEFORE the tracker and the replacement pass of frame t and the GPU overlaps
 * them (one event each way per frame).  0 (default): one stream.  The caller must give frame t+1 a slot that no call still to be
 * enqueued reads (a ring of three slots for a sequence). */
#define KLT_OPT_BUILD_STREAM 15
#define KLT_OPT_TRACK_TREE_SUMS 18        /* (does not apply to klt_track_fb*, which always add in the reference's order) 0 (default): the tracker adds its five window sums (and the residue) in the reference's order -- records identical to the reference's bit for bit; 1: butterfly sums in registers (7x7 / 15x15 quad kernels; same precision, other order of the additions): positions agree to 1e-3 px, a status word can differ where a feature sits on a threshold */
#define KLT_OPT_SCORE_SETS 16            /* how many sets of prepared selection scores (klt_select_prepare_async) the context keeps: 2 (default) .. 256; a selection frees the set it uses */
/* 1 .. 8 (default 2; KLT_COPY_STREAMS in the environment sets the initial value): the copy streams consecutive klt_upload_u8_async calls
 * alternate between.  Two let the frames of a PAIR travel side by side (45 GB/s against 28-39 on one or three); a SEQUENCE loop -- one new
 * frame per step -- is faster on ONE (0.280 against 0.307 ms per 4K frame, 0.141-0.152 against 0.148-0.155 at 1080p: with two, the host's look
 * at every other frame's selection waits 211 instead of 102 us, profiles/README.md): KLTTrackSequence and bench.py's sequence loops set 1. */
#define KLT_OPT_COPY_STREAMS 20
/* test hook: >= 0: the library's (value + 1)-th device / pinned-host allocation from now is refused as if memory had run out (KLT_ERR_NOMEM; the
 * context stays usable, the call can be repeated); -1 (default): off.  Lets the tests walk every allocation site of a call sequence. */
#define KLT_OPT_FAIL_ALLOC_AFTER 19
/* 1: the level-0 kernel with the fused first reduction walks each 64-column strip down in bands and computes every row of every
 * stage once (frames of >= 128 columns); 0: the tiled kernel, which computes each tile's vertical halo again; 2 (default): as 1, on 128-column
 * strips in 16-row bands where the launch has >= 256 columns and fills the chip with them (fewer halo columns smoothed per output column),
 * else as 1.  Same results bit for bit. */
#define KLT_OPT_L0_STREAM 21
/* Level-0 gradients on demand.  A LEAN build of a slot launches the streaming level-0 kernel without its gradient passes: it writes the
 * smoothed image to a compact f32 plane of the slot (4 bytes per pixel, allocated on the slot's first lean build and freed with the slot,
 * on top of the 12 bytes per pixel of the level's records) and leaves the level-0 records unwritten; levels >= 1 are built as ever.  The
 * plain 7x7 quad tracker (klt_track_async, klt_track_batch_async; lists of features x pairs >= 2048, default KLT_OPT_TRACK_VARIANT, sums in
 * the reference's order, no lighting compensation) then makes the gradients of the footprints it visits itself, from that plane.  Whatever
 * else reads level 0 of a lean slot -- every other tracker, a launch that mixes slots with and without a compact plane, selection, score
 * preparation, quality, the affine check, klt_download_f32 -- first gets the records made from the compact plane by the gradient launch of
 * the levels >= 1.  Records, planes and every result are the same bit for bit either way.
 *   0: never lean.
 *   1 (default): a slot is built lean when, since its previous build, such a tracker launch read it and nothing asked for its level-0
 *      records -- so a slot's first build is full, a flow that selects or checks on every frame stays full, and a flow that only tracks
 *      resident or streamed frames goes lean from its second build on.
 *   2: always lean where a streaming kernel is launched (for tests). */
#define KLT_OPT_L0_LAZY_GRAD 22
/* Which kernel a lean launch takes.  1: the wave form (smooth_grad_lean_wave: a wavefront owns a 232-column strip and walks it down a
 * segment of KLT_L0_LEAN_WAVE_SEG rows on its own, no workgroup barrier) where the frames have >= 256 columns and at least as many rows
 * as smoothing taps, the banded form elsewhere; 0: always the banded form (the streaming kernel without its gradient passes).  Which
 * builds go lean does not depend on it, and the planes are the same bit for bit. */
#define KLT_OPT_L0_LEAN_FORM 23
#define KLT_L0_LEAN_FORM_DEFAULT 1
/* How the tracker that makes its level-0 gradients itself (KLT_OPT_L0_LAZY_GRAD) enters level 0.  1: one fused phase makes the gradients
 * of the template's footprint and of the first search footprint together -- the image patches of both are requested before anything waits
 * for either, each patch row is filtered by one lane; 0: one phase per footprint, one after the other.  Footprints that a Newton step moves
 * to another pixel are recomputed one at a time in both forms.  Same results bit for bit. */
#define KLT_OPT_TRACK_LAZY_FORM 24
#define KLT_TRACK_LAZY_FORM_DEFAULT 1
#define KLT_L0_LEAN_WAVE_SEG 32     /* segment height of the wave form, rows (pyfeaturetrack_amd/_abi.py carries the same figure) */
int klt_set_option(klt_ctx *ctx, int option, int value);

/* ---- parameters and taps ------------------------------------------------------------------- */
int klt_set_params(klt_ctx *ctx, const klt_params *p);      /* klt.py:45-73, :84-128, :137-189 */
/* FP64 taps computed on the host exactly as convolve.py:27-93 (_computeKernels).
 * which: 0 = smoothing (sigma = smooth_sigma_fact*max(w,h)), 1 = pyramid (pyramid_sigma_fact*ss), 2 = gradient (grad_sigma) */
int klt_set_kernels(klt_ctx *ctx, int which, const double *gauss, int ng, const double *deriv, int nd);

/* ---- frames (slots) ------------------------------------------------------------------------ */
/* replaces `np.array(img.convert("F"))`, trackFeatures.py:165,176 / selectGoodFeatures.py:190.
 * pitch is in elements.  The upload is enqueued; the host buffer may be reused on return.
 * Limits: 1 <= ncols, nrows <= 65535 and ncols * nrows < 2^27 (the kernels address a plane with 32-bit byte offsets below 2 GB, and
 * the pixel-record plane of level 0 has 12 bytes per pixel); a frame
 * beyond them is KLT_ERR_ARG here, at klt_upload_u8_async and at the stand-alone convolution / pyramid calls. */
int klt_upload_u8(klt_ctx *ctx, int slot, const uint8_t *px, int ncols, int nrows, int pitch);
int klt_upload_f32(klt_ctx *ctx, int slot, const float *px, int ncols, int nrows, int pitch);
/* Asynchronous ingest: the frame is copied from PINNED host memory on a dedicated copy stream and overlaps
 * the kernels of earlier frames; the next build / selection of the slot waits for it on the device, the copy itself
 * waits for queued work that still reads the slot.  `px` must stay untouched until klt_upload_wait (or klt_sync) has
 * returned after the call. */
int klt_host_alloc(klt_ctx *ctx, size_t bytes, void **out);     /* pinned host memory, freed by klt_host_free / klt_destroy */
int klt_host_free(klt_ctx *ctx, void *p);
int klt_upload_u8_async(klt_ctx *ctx, int slot, const uint8_t *px, int ncols, int nrows, int pitch);
/* the same for a float32 frame (what `img.convert("F")` of a colour or float image gives, trackFeatures.py:165,176): pinned host memory,
 * copy streams, the slot's two alternating raw buffers -- 4 bytes per pixel on the link */
int klt_upload_f32_async(klt_ctx *ctx, int slot, const float *px, int ncols, int nrows, int pitch);
int klt_upload_wait(klt_ctx *ctx);      /* host waits for the copies issued so far (only the copy stream; kernels keep running) */
/* Host side of the ingest, no context involved (thread-safe; a process-wide pool of parked worker threads, KLT_HOST_THREADS lanes in
 * all, default 4; a caller that finds the pool busy does its own work): the reference converts and rebuilds both images on every call
 * (trackFeatures.py:146-196); a caller that keeps a frame's pyramids while the image still has EXACTLY the pixels the slot was filled
 * from pays one pass over the frame per call instead -- klt_host_compare: 0 = every byte equal, 1 = different --, and stages a new
 * frame into the pinned buffer klt_upload_u8_async reads with klt_host_copy. */
int klt_host_compare(const void *a, const void *b, size_t bytes);
int klt_host_copy(void *dst, const void *src, size_t bytes);
int klt_host_lanes(void);               /* lanes a large compare / copy is spread over (workers + the caller) */
/* The same two for a frame that is NOT one contiguous array but a table of row addresses -- Pillow's ImagingMemoryInstance.image8, which the
 * reference's callers hand in (trackFeatures.py:165,176 / selectGoodFeatures.py:190: `img.convert("F")` of a PIL image; the Python layer
 * takes the table from Image.getim(), pyfeaturetrack_amd/_pil.py): rows[r] = address of row r, row_bytes bytes each; `b` / `dst` a contiguous
 * [nrows x row_bytes] buffer (the pinned copy a slot was filled from).  Rows that follow each other in memory are treated as one range.
 * klt_host_sample_rows: rows[y][x] for y = 0, ystep, ... and x = 0, xstep, ... (row-major) into out; returns the count (the 1024-pixel
 * lattice of the frame cache without making an array of the image). */
int klt_host_compare_rows(const uint8_t *const *rows, int nrows, size_t row_bytes, const void *b);
int klt_host_copy_rows(void *dst, const uint8_t *const *rows, int nrows, size_t row_bytes);
/* on != 0: compares / copies issued by the CALLING THREAD from now on stay on that thread (a background thread that stages frames while
 * the main thread enqueues must not take the pool's lanes away from it: measured slower, profiles/README.md); returns the previous setting */
int klt_host_thread_serial(int on);
int klt_host_sample_rows(const uint8_t *const *rows, int nrows, int ncols, int ystep, int xstep, uint8_t *out, size_t cap);
/* `img.convert("F")` of a colour image without Pillow's intermediate image and numpy's copy of it: rows of 4-byte pixels (R, G, B, X --
 * Pillow's storage of "RGB" / "RGBA" / "RGBX" images, ImagingMemoryInstance.image32) -> dst[nrows][ncols] float32 =
 * (float)(299 R + 587 G + 114 B) / 1000.0f, Pillow's own expression (libImaging/Convert.c, rgb2f), spread over the pool's lanes */
int klt_host_luma_rows(float *dst, const uint8_t *const *rows, int nrows, int ncols);
/* Frames that are ALREADY in device memory (a hardware decoder's output, a clip kept resident): the slot's frame becomes this caller-owned
 * buffer -- read in place by the next build / selection of the slot, never copied, written or freed by the library (zero-copy
 * ingest).  pitch must equal ncols.  The address needs no alignment: a frame may start at any byte (frame k of a clip at clip + k * size,
 * or behind a header of any length); frames on a multiple of 4 bytes whose width is divisible by 4 take the level-0 kernels' 4-byte
 * loads, every other frame is read byte by byte, with the same planes.  Host-only call: nothing is enqueued; the buffer must hold the frame already and stay unchanged until
 * the work that reads it has completed (klt_sync, or the download of what was computed from it).  The next upload into the slot ends the
 * adoption.  klt_device_alloc / klt_device_write / klt_device_free give callers without a HIP binding of their own (Python) such memory:
 * owned by the context, freed with it. */
int klt_slot_adopt_u8(klt_ctx *ctx, int slot, const uint8_t *dev_px, int ncols, int nrows, int pitch);
int klt_device_alloc(klt_ctx *ctx, size_t bytes, void **out);
int klt_device_write(klt_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);   /* synchronous host-to-device copy */
int klt_device_free(klt_ctx *ctx, void *dev);
/* smooth -> pyramid -> gradients of every level: ComputeImagePyramids for one image,
 * trackFeatures.py:165-172 + pyramid.py:37-77 + convolve.py:208-264 */
int klt_build_pyramids_async(klt_ctx *ctx, int slot);
/* the same for several slots at once: frames of equal size share kernel launches (both frames of a pair,
 * or every pair of a batch -- BASELINE cfg-4) */
int klt_build_pyramids_batch_async(klt_ctx *ctx, const int *slots, int n);
int klt_build_pyramids(klt_ctx *ctx, int slot);
/* Diagnostic, read-only: which kernel the most recent klt_build_pyramids* call launched for level 0 of its LAST group of frames (frames of
 * one size and input type share launches, at most 32 per group) -- one of the KLT_L0_* codes, recorded where the launch decision is made;
 * KLT_ERR_STATE before the first build.  *merged_grad (may be NULL): 1 when the gradients of that group's levels >= 1 went out as ONE
 * launch with per-entry geometry (frames x (levels - 1) <= 32), 0 when each level had a launch of its own.  The choice depends on the
 * launch's size, the taps, the subsampling and KLT_OPT_FUSED_KERNELS / KLT_OPT_FUSED_HREDUCE / KLT_OPT_L0_STREAM; every path gives the
 * same planes bit for bit -- the tests use this to know that the kernel they were written for is the one that ran. */
#define KLT_L0_TWO_PASS 0           /* generic two-pass convolution kernels (KLT_OPT_FUSED_KERNELS 0, asymmetric smoothing taps) */
#define KLT_L0_TILED_LDS 1          /* smooth_grad_kernel: LDS-tiled, taps of any count */
#define KLT_L0_RB16 2               /* smooth_grad_rb, 16-row tiles (launches below 1 000 000 pixels) */
#define KLT_L0_RB32 3               /* smooth_grad_rb, 32-row tiles */
#define KLT_L0_RB32_HRED 4          /* 32-row tiles with the first reduction's horizontal pass (KLT_OPT_FUSED_HREDUCE) */
#define KLT_L0_STREAM 5             /* smooth_grad_stream (KLT_OPT_L0_STREAM), f32 frames */
#define KLT_L0_STREAM_NO_CENTRE 6   /* smooth_grad_stream with the derivative taps' centre product elided (u8 frames) */
#define KLT_L0_STREAM_WIDE 7        /* smooth_grad_stream on 128-column strips in 16-row bands (KLT_OPT_L0_STREAM 2), f32 frames */
#define KLT_L0_STREAM_WIDE_NO_CENTRE 8  /* ... with the centre product elided (u8 frames) */
int klt_level0_path(klt_ctx *ctx, int *merged_grad);
/* *lean = 1 if the last geometry group of the last build went out lean (KLT_OPT_L0_LAZY_GRAD; klt_level0_path reports the code of the
 * streaming geometry as for a full launch), else 0.  KLT_ERR_STATE before the first build. */
int klt_level0_lean(klt_ctx *ctx, int *lean);
/* *form = which kernel that group's level-0 launch was: 0 not lean, 1 the banded lean form, 2 the wave form (KLT_OPT_L0_LEAN_FORM).
 * KLT_ERR_STATE before the first build. */
int klt_level0_lean_form(klt_ctx *ctx, int *form);
/* bit 0: the slot holds a frame; bit 1: its pyramids are built and match the current parameters / taps (what
 * `tc.pyramid_last is not None` means in the reference, trackFeatures.py:152); 0 for a slot never used */
int klt_slot_state(klt_ctx *ctx, int slot);
/* free / total memory of the context's device (hipMemGetInfo): what a long-running sequence watches to see that slots, score sets and
 * descriptor tables are recycled, not accumulated */
int klt_device_memory(klt_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
/* which build filled the slot's pyramids: a number unique per build within the context that travels with klt_swap_slots; 0 while the
 * slot has no valid pyramids.  The host layer's pyramid handles (what ComputeImagePyramids returns and tc.pyramid_last holds,
 * trackFeatures.py:146-196, :401-404) use it to tell whether the planes they stand for are still on the device. */
int klt_slot_generation(klt_ctx *ctx, int slot, uint64_t *gen);
/* releases the slot's device memory (raw frames, pyramids); the index can be used again.  The reference frees images and
 * pyramids when the Python objects die; the host layer calls this from a finalizer of the tracking context. */
int klt_slot_free(klt_ctx *ctx, int slot);
/* sequentialMode: the frame-2 pyramids become frame 1 (trackFeatures.py:152-161, :401-404) */
int klt_swap_slots(klt_ctx *ctx, int a, int b);

/* ---- feature buffers ----------------------------------------------------------------------- */
int   klt_featbuf_upload(klt_ctx *ctx, int fb, const klt_feat *src, int n);
/* the same without waiting for the copy: `src` must stay untouched until the next synchronising call on the context (klt_sync,
 * klt_featbuf_download, ...) */
int   klt_featbuf_upload_async(klt_ctx *ctx, int fb, const klt_feat *src, int n);
int   klt_featbuf_download(klt_ctx *ctx, int fb, klt_feat *dst, int n);
/* the same without draining the pipeline: the copy is enqueued in stream order behind the kernels that wrote the records; `dst` must be
 * pinned (klt_host_alloc) and holds the records once klt_download_wait (or any synchronising call) has returned.  A loop that reads a
 * table back every N steps issues this at the window's end and waits for it at the NEXT window's end: the host never waits for queued work. */
int   klt_featbuf_download_async(klt_ctx *ctx, int fb, klt_feat *dst, int n);
int   klt_download_wait(klt_ctx *ctx);                        /* host waits for the latest klt_featbuf_download_async / klt_download_mark_async */
/* marks this point of the main stream for klt_download_wait without copying anything: for records the kernels write straight into pinned
 * memory (klt_featbuf_map_host) when more work is enqueued behind the kernel that writes them -- KLTTrackFeatures (trackFeatures.py:205-409)
 * waits for its tracker only while the scores of the KLTReplaceLostFeatures call that follows are already being computed */
int   klt_download_mark_async(klt_ctx *ctx);
/* Feature buffer `fb` becomes `n` records of PINNED host memory (klt_host_alloc), read and written in place by the kernels over the
 * link: a call that sends a list, tracks it and waits (KLTTrackFeatures, trackFeatures.py:205-409) then needs no copy command in either
 * direction -- the records are in `host` once klt_sync (or any synchronising call) has returned.  Meant for the lists of such one-shot
 * calls; tables that kernels revisit belong in device memory.  host == NULL ends the mapping (the buffer is empty afterwards).  The
 * memory must outlive the mapping. */
int   klt_featbuf_map_host(klt_ctx *ctx, int fb, klt_feat *host, int n);
int   klt_featbuf_alloc(klt_ctx *ctx, int fb, int n);         /* n records, all marked lost (val = -1) */
/* fb_view becomes a window [offset, offset+n) of fb_parent (a device-side [frames x features] table, cf. the
 * KLT_FeatureTable stub at klt.py:278-283, can then be gathered with one collective).  The parent must outlive the
 * view and must not be resized while it exists. */
int   klt_featbuf_view(klt_ctx *ctx, int fb_view, int fb_parent, int offset, int n);
void *klt_featbuf_devptr(klt_ctx *ctx, int fb);             /* device address (for RCCL gathers); NULL if unset */

/* ---- selection: _KLTSelectGoodFeatures, selectGoodFeatures.py:141-261 ---------------------- */
/* ScanImageForGoodFeatures (goodFeaturesUtils.pyx:35-73) + sort (:234-236) + _enforceMinimumDistance
 * (:45-135).  mode KLT_REPLACING_SOME keeps features with val >= 0.  If use_pyramid != 0 the
 * level-0 image/gradients of the slot's pyramids are reused (selectGoodFeatures.py:176-181),
 * otherwise the slot's raw frame is smoothed/differentiated afresh (:183-197). */
int klt_select_async(klt_ctx *ctx, int slot, int mode, int use_pyramid, int fb, int n);
/* klt_select_async in two halves.  klt_select_begin_async enqueues everything up to the point where the host has to look at the
 * outcome (how many passes the minimum-distance stage needed, whether the candidate cut held); klt_select_finish waits, looks and --
 * rarely -- enqueues more passes or the repeat with every candidate.  Between the two the caller may enqueue other work that does not
 * WRITE the list or select again: the next frame's upload, build and klt_select_prepare_async (a sequence overlaps the host side of
 * frame t+1 with the GPU side of frame t's replacement this way) -- and work that only READS the list, such as the tracker launch of the
 * next frame into another buffer (klt_track_async: the GPU then has the tracker queued while the host looks at the outcome and enqueues
 * the next selection, instead of idling through that turn-around).  klt_select_finish returns KLT_OK, or 1 (not an error) when it had to
 * rewrite the list after the launches of klt_select_begin_async had run (more passes, or the repeat with every candidate): whatever
 * read the list in between must then be enqueued again.  klt_select_finish without a pending selection returns KLT_OK. */
int klt_select_begin_async(klt_ctx *ctx, int slot, int mode, int use_pyramid, int fb, int n);
int klt_select_finish(klt_ctx *ctx);
/* The list-independent half of a later klt_select_async(slot, KLT_REPLACING_SOME, use_pyramid = 1, ...): the summed-area tables and
 * the eigenvalue of every candidate window (goodFeaturesUtils.pyx:17-73, called from selectGoodFeatures.py:199-232) of the slot's
 * level-0 gradients, kept with the slot's contents (KLT_OPT_SCORE_SETS sets per context; a set follows klt_swap_slots, is used by one
 * selection, and dies with the next build
 * of the slot or a change of the selection parameters).  With KLT_OPT_BUILD_STREAM it runs on the build stream, i.e. while the main
 * stream tracks into the previous frame and replaces its lost features; the selection then only masks the live features'
 * squares, cuts and runs the minimum-distance passes.  Same result with or without this call. */
int klt_select_prepare_async(klt_ctx *ctx, int slot);
int klt_select(klt_ctx *ctx, int slot, int mode, int use_pyramid, klt_feat *inout, int n, int *n_placed);
/* Selection mask: where klt_select* may NOT place features (a vehicle's bonnet, a burnt-in timestamp, the sky, moving objects found by a
 * segmentation network).  [nrows][ncols] bytes, state of the context like the parameters: a pixel whose byte is 0 is never a candidate,
 * any other value leaves it eligible.  The selection is exactly what it would be had ScanImageForGoodFeatures never put the masked
 * positions on the point list _enforceMinimumDistance walks (selectGoodFeatures.py:45-135, :230-236); nothing else changes: in
 * KLT_REPLACING_SOME live features inside masked areas are kept and still block their squares; the tracker, klt_min_distance_walk,
 * klt_scan_good_features_f32 and klt_select_prepare_async ignore the mask (prepared scores depend on neither list nor mask: the selection
 * that uses them applies it); with klt_set_score_override both apply and the mask wins; in klt_download_select_f32(what = 3) masked
 * candidates read 0.  A context without a mask enqueues nothing for it.
 * klt_set_select_mask copies a HOST mask (pitch in bytes >= ncols) into a device plane the context owns before it returns.
 * klt_set_select_mask_device takes a mask that is ALREADY in device memory (a network's output; klt_device_alloc / klt_device_write for
 * callers without a HIP binding): rows without padding (pitch == ncols, cf. klt_slot_adopt_u8), the address a multiple of 16
 * (KLT_ERR_ARG otherwise); it is read in place -- never a byte behind ncols * nrows -- and never written or freed by the library.
 * mask == NULL / dev_mask == NULL removes the mask (the sizes are not looked at).
 * When it is read: once per selection, in stream order, by a kernel klt_select_begin_async enqueues (klt_select_async and klt_select
 * go through it); a repeat inside klt_select_finish (more passes, the fallback to every candidate) does not read it again.  The
 * contents of a device mask may therefore be changed as soon as klt_select_begin_async has returned and the stream has passed that
 * point (klt_device_write, or a kernel enqueued behind it on klt_stream_handle).  The mask ITSELF cannot be set or removed while a
 * selection is pending: KLT_ERR_STATE between klt_select_begin_async and klt_select_finish.
 * A mask whose size differs from the frame of the slot a selection is asked for makes that klt_select* call return KLT_ERR_ARG (the
 * message names both sizes) before it enqueues anything; the mask stays set and the context usable.  A klt_set_select_mask that fails
 * (KLT_ERR_NOMEM for the plane) leaves the context WITHOUT a mask, and so does klt_device_free of the allocation a device mask
 * lives in. */
int klt_set_select_mask(klt_ctx *ctx, const uint8_t *mask, int ncols, int nrows, int pitch);
int klt_set_select_mask_device(klt_ctx *ctx, const uint8_t *dev_mask, int ncols, int nrows);
/* Selection grid: a cap on how many features one image cell may hold (grid-balanced selection, as visual-odometry front ends bucket their
 * features).  Cells are cell_width x cell_height PIXELS; on an ncols x nrows frame there are gw = ceil(ncols / cell_width) by
 * gh = ceil(nrows / cell_height) of them (the last column and row may be narrower) and pixel (x, y) lies in cell
 * (y / cell_height) * gw + x / cell_width.  State of the context like the mask and the parameters, and independent of the frame size.
 * The rule, composed from _enforceMinimumDistance (selectGoodFeatures.py:45-135): let A = (a_1, a_2, ...) be the candidates the walk
 * accepts, in the order it accepts them, if the list were never full (in KLT_REPLACING_SOME the squares of the live features are marked
 * first, as always).  Without a grid the selection is the first `free slots` members of A.  With a grid, cap(c) = max_per_cell in
 * KLT_SELECTING_ALL and max(max_per_cell - live(c), 0) in KLT_REPLACING_SOME, where live(c) counts the list's records with val >= 0 whose
 * position passes 0 <= x < ncols && 0 <= y < nrows as f32 comparisons (a NaN fails) in the cell of ((int)x, (int)y); a_i is KEPT iff it
 * is among the first cap(cell(a_i)) members of A in its cell, and the free slots (every slot when overwriting, else the lost ones) are
 * filled in list order with the kept members in order, until slots or members run out.  Slots of a KLT_SELECTING_ALL the members did
 * not reach become (-1, -1, KLT_NOT_FOUND), as without a grid.  Live features are never removed, even where a cell holds more than
 * max_per_cell of them.  A member of A that is not kept STILL excludes its neighbours: A does not depend on the grid, and the grid never
 * admits a weaker neighbour of a stronger corner it turned away.
 * klt_min_distance_walk, klt_scan_good_features_f32, klt_select_prepare_async and the tracker ignore the grid; the mask and
 * klt_set_score_override act on the point list, the grid on A, so they compose; KLT_OPT_SELECT_AFFINE_STATE resets exactly the slots that
 * are filled.  A context without a grid enqueues nothing for it.
 * g == NULL or g->cell_width == 0 removes the grid (the default).  KLT_ERR_ARG for cell_width or cell_height < 1 or max_per_cell outside
 * 1 .. 65535; KLT_ERR_STATE between klt_select_begin_async and klt_select_finish.
 * klt_select_grid_path: how the last selection under a grid applied it -- 0: none has run yet; 1: a filter kernel between the parallel
 * minimum-distance passes and the placement by rank; 2: the quota inside the greedy walk (KLT_OPT_SELECT_PARALLEL_NMS = 0, exclusion
 * squares too large for the passes, more accepted candidates than the ranking takes, or max_per_cell above 64). */
typedef struct { int32_t cell_width, cell_height, max_per_cell; } klt_select_grid;
int klt_set_select_grid(klt_ctx *ctx, const klt_select_grid *g);
int klt_select_grid_path(klt_ctx *ctx);
/* replaces _enforceMinimumDistance(pointlist, featurelist, ncols, nrows, mindist, min_eigenvalue, overwriteAllFeatures) called on its own
 * (selectGoodFeatures.py:45-135): the greedy walk over a GIVEN candidate list in the GIVEN order.  keys[i] = f32 bits of val << 32 |
 * x << 16 | y (what klt_download_sorted_candidates returns, re-packed); the caller has dropped the candidates the walk skips without
 * effect (val < min_eigenvalue; positions inside the (2 mindist - 1)-squares of live features when overwrite_all == 0).  Free slots of
 * `inout` are filled in list order -- every slot by rank when overwrite_all, the lost ones (val < 0) otherwise; with overwrite_all the
 * slots the candidates did not reach become (-1, -1, KLT_NOT_FOUND).  Every candidate must lie inside the image (x < ncols, y < nrows;
 * KLT_ERR_ARG otherwise, checked here: the reference asserts the same, :90-91) and no key may be zero (value 0.0 at (0, 0): the walk's own
 * end mark; the reference never accepts a value below 1, :95).  Synchronous; needs no parameters and no frame. */
int klt_min_distance_walk(klt_ctx *ctx, const uint64_t *keys, int nkeys, int ncols, int nrows, int mindist, int overwrite_all,
                          klt_feat *inout, int n, int *n_placed);

/* ---- tracking: KLTTrackFeatures, trackFeatures.py:205-409 (translation model) -------------- */
/* _trackFeature (:67-136) + trackFeatureIterateCKLT (trackFeaturesUtils.pyx:393-459) for every
 * live feature, coarse to fine, one wavefront per feature.  Pyramids of both slots must be built. */
int klt_track_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_out, int n);
int klt_track(klt_ctx *ctx, int slot1, int slot2, klt_feat *inout, int n, int *n_tracked);
/* npairs independent frame pairs of equal size in ONE tracker launch (BASELINE cfg-4: a shard of the 256 pairs);
 * pair i tracks feature buffer fb_in[i] (n records) from slot1[i] to slot2[i] into fb_out[i] */
int klt_track_batch_async(klt_ctx *ctx, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out,
                          int npairs, int n);

/* ---- forward-backward consistency check (not in the reference) ------------------------------------------ */
/* Let T(a, b, list) be what klt_track_async(slot_a, slot_b, ...) gives for `list`.  fwd = T(1, 2, in); back = T(2, 1, fwd) (records of
 * fwd with val < 0 pass through, as always).  A feature that was live in `in` and has fwd.val == KLT_TRACKED is CONSISTENT iff
 * back.val == KLT_TRACKED and (double)dx*(double)dx + (double)dy*(double)dy <= (double)max_error*(double)max_error with the f32 differences
 * dx = back.x - in.x, dy = back.y - in.y (exact products, one rounding in the sum).  out = fwd for a consistent feature (the whole record),
 * (-1, -1, KLT_FB_INCONSISTENT, fwd.aux) for an inconsistent one, and exactly T(1, 2, in) for every other record.  One kernel launch does
 * both descents of a feature; it always uses the reference-order window sums (KLT_OPT_TRACK_TREE_SUMS is not looked at), so `out` and
 * `back` equal the composition of two default klt_track_async calls bit for bit, for every window and KLT_OPT_TRACK_VARIANT.
 * Stateless; not offered together with the affine check (klt_track_affine_async is untouched). */
typedef struct { int32_t enabled; float max_error; } klt_fb_params;
/* max_error in pixels (default 1.0), negative or NaN: KLT_ERR_ARG.  `enabled` is kept for the host layer (the Python API reads the
 * tracking context's flag); the klt_track_fb* calls below run the check whenever they are called. */
int klt_set_fb_params(klt_ctx *ctx, const klt_fb_params *p);
/* fb_back: feature buffer that receives `back` (n records), or -1.  fb_in, fb_out and fb_back must be pairwise distinct. */
int klt_track_fb_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_out, int n, int fb_back);
int klt_track_fb(klt_ctx *ctx, int slot1, int slot2, klt_feat *inout, klt_feat *back_or_NULL, int n, int *n_tracked);
/* npairs pairs in one launch (cf. klt_track_batch_async); fb_back may be NULL (no pair's backward records are kept) and single entries -1 */
int klt_track_fb_batch_async(klt_ctx *ctx, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out, const int *fb_back,
                             int npairs, int n);

/* ---- motion prior: start each feature's search from a predicted position (not in the reference) ---------- */
/* `guess` is a list of klt_feat records next to `in`, same index = same feature: x, y = the predicted position in frame 2.  For a live
 * feature (in.val >= 0) the guess COUNTS iff guess.val >= 0 and guess.x and guess.y are both finite.  The only thing that changes is where
 * the coarse-to-fine loop (trackFeatures.py:250-346) starts its search: with a guess that counts xlocout = guess.x / ss^L and
 * ylocout = guess.y / ss^L (exact divisions, as for xloc), without one xlocout = xloc as in klt_track_async.  The template position, the
 * per-level bounds tests, the status priority, the border test and the aux bits are klt_track_async's.  A finite guess outside the image
 * is caught by the first level's bounds test: KLT_OOB, which is what the reference says about a search position outside the image.
 * Records are identical bit for bit to klt_track_async's when every guess is the feature's own position or none counts (every window,
 * KLT_OPT_TRACK_VARIANT, KLT_OPT_TRACK_XCD_ORDER and KLT_OPT_TRACK_TREE_SUMS value).
 * fb_guess must hold at least n records and be distinct from fb_out (and fb_back): KLT_ERR_ARG otherwise.  It may be fb_in. */
int klt_track_guess_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_guess, int fb_out, int n);
int klt_track_guess(klt_ctx *ctx, int slot1, int slot2, klt_feat *inout, const klt_feat *guess, int n, int *n_tracked);
/* npairs pairs in one launch (cf. klt_track_batch_async); a fb_guess entry of -1: that pair has no guess list.  A pair's guess list must be
 * distinct from every pair's fb_out. */
int klt_track_guess_batch_async(klt_ctx *ctx, const int *slot1, const int *slot2, const int *fb_in, const int *fb_guess, const int *fb_out,
                                int npairs, int n);
/* The forward-backward check with a prior: fwd = G(1, 2, in, guess), back = T(2, 1, fwd) -- the way back starts at the forward result as
 * in klt_track_fb_async (a prior there would bias the check) -- then the rule above.  Reference-order sums, like klt_track_fb*. */
int klt_track_fb_guess_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_guess, int fb_out, int n, int fb_back);
/* Constant-velocity prediction from the lists of the last two frames: for a slot with cur.val == KLT_TRACKED and prev.val >= 0
 * guess = (cur.x + (cur.x - prev.x), cur.y + (cur.y - prev.y), 0, 0), each coordinate two f32 roundings; every other slot -- lost, or
 * refilled by a replacement pass (val > 0) -- gets (-1, -1, -1, 0): no guess.  fb_guess is allocated if needed and may be neither of the
 * other two (KLT_ERR_ARG). */
int klt_predict_cv_async(klt_ctx *ctx, int fb_prev, int fb_cur, int fb_guess, int n);

/* ---- gain / bias (lighting-insensitive) tracking (not in the reference as code) ------------------------------ */
/* KLT 1.3.4's lighting-insensitive Newton step, which the reference carries as commented text (trackFeaturesUtils.pyx:152-239) and calls
 * for at trackFeatures.py:119-120.  Per level and feature, with T / S the window samples of image 1 / of image 2 at the current position,
 * n samples, nf = (float)n, all sums sequential f32 chains in row-major order: sum1 = SUM T, sq1 = SUM T*T, sum2 = SUM S, sq2 = SUM S*S;
 * alpha = (float)sqrt((double)((sq1/nf) / (sq2/nf))), beta = sum1/nf - alpha*(sum2/nf), diff = (T - S*alpha) - beta;
 * alpha_g = (float)sqrt((double)((sum1/nf) / (sum2/nf))) (the ratio of the means, as KLT 1.3.4 has it), gradient sums Tg + Sg*alpha_g;
 * everything else -- the five product sums, the solve, step factor, bounds tests, iteration cap, status priority, retainTrackers, border
 * rule, aux word -- is klt_track_async's; the residue is taken from |diff| with alpha and beta of the final position.  A window whose
 * sums are not all positive and finite, or whose alpha / alpha_g (or Newton step) is not finite, ends its level with KLT_SMALL_DET at the
 * position it has.  With mode 1 klt_track, klt_track_async and klt_track_batch_async launch these kernels (features in list order:
 * KLT_OPT_TRACK_XCD_ORDER and KLT_OPT_TRACK_TREE_SUMS are not looked at); klt_track_fb*, klt_track_guess*, klt_track_fb_guess_async and
 * klt_track_affine* return KLT_ERR_STATE before anything is enqueued.  With mode 0 nothing changes. */
typedef struct { int32_t mode; } klt_light_params;   /* 0 off (default), 1 gain + bias */
int klt_set_light_params(klt_ctx *ctx, const klt_light_params *p);          /* another mode: KLT_ERR_ARG */
/* which kernel the last launch with mode 1 took -- 0: no such launch yet, 1: one feature per wavefront, 2: four 7x7 features per wavefront
 * (7x7 windows, features x pairs >= 2048, KLT_OPT_TRACK_VARIANT != 0).  A diagnostic: both give the same records. */
int klt_track_light_path(klt_ctx *ctx);

/* ---- per-feature track quality (not in the reference) --------------------------------------------------------- */
/* One launch that reads two feature lists and level 0 of two slots and writes one 16-byte quality record per feature; it decides
 * nothing and changes nothing else.  With in / out record i of the two lists, w = window_width, n = w * w, hw = w / 2:
 *   measured   in.val >= 0 and out.val == KLT_TRACKED (a slot refilled by a replacement pass, val > 0, is not measured), both positions
 *              0 <= x < ncols and 0 <= y < nrows (NaN and infinities fail; tested before any conversion to int), both windows inside
 *              the frame by the sampler's own test (ix-hw >= 0, iy-hw >= 0, ix+hw+2 <= ncols, iy+hw+2 <= nrows, ix = (int)x).  Every other
 *              record is (0, 0, 0, val = 0); a measured one has val = 1.
 *   samples    T of frame 1's level-0 image at (in.x, in.y); S, Sgx, Sgy of frame 2's image and gradients at (out.x, out.y), the
 *              tracker's bilinear samples, k row-major over the window.
 *   residue    SUM |T_k - S_k| (f32 terms, numpy's pairwise f32 sum) / (float)n: the number klt_params.max_residue tests
 *              (trackFeatures.py:124).
 *   ncc        the normalised cross-correlation of T and S from FP64 sums of exact products (term k joins partial k mod 64 in
 *              increasing k, the partials fold by p[l] += p[l + m], l < m, m = 32 .. 1): a = n*SUM TT - (SUM T)^2, b = n*SUM SS - (SUM S)^2,
 *              c = n*SUM TS - SUM T * SUM S, every operation one FP64 rounding; a > 0 && b > 0: (float)clamp(c / sqrt(a*b), -1, 1), else 0.
 *              A gain and an offset between the frames leave it alone, where they make the residue meaningless.
 *   min_eig    the smaller eigenvalue of the window's gradient matrix at the new position, from the same kind of sums gxx, gxy, gyy of
 *              Sgx, Sgy: d = gxx - gyy, (float)max(((gxx + gyy) - sqrt(d*d + 4*(gxy*gxy))) / 2, 0).
 * Quality records live in feature buffers (size and alignment of klt_feat): views, downloads, table rows and gathers work unchanged.
 * Any odd window 3 .. 31.  The launches do not look at the forward-backward, lighting or affine parameters. */
typedef struct { float residue, ncc, min_eig; int32_t val; } klt_quality;
/* Both pyramids built (KLT_ERR_STATE) and of equal size (KLT_ERR_ARG), fb_in and fb_out hold n records (KLT_ERR_STATE); fb_quality is
 * allocated if needed and distinct from fb_in and fb_out, by index and by address (KLT_ERR_ARG).  n == 0: KLT_OK, nothing enqueued. */
int klt_track_quality_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_out, int fb_quality, int n);
/* npairs pairs of equal frame size in one launch; every fb_quality distinct from every pair's fb_in and fb_out, and from each other */
int klt_track_quality_batch_async(klt_ctx *ctx, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out,
                                  const int *fb_quality, int npairs, int n);
/* synchronous, host arrays: q[i] from in[i] and out[i] */
int klt_track_quality(klt_ctx *ctx, int slot1, int slot2, const klt_feat *in, const klt_feat *out, klt_quality *q, int n);

/* ---- motion-model check (not in the reference) ------------------------------------------------------------------ */
/* Judges every track of a frame pair against the other tracks of that pair: a seeded consensus search for the pair's dominant affine
 * motion, one least-squares refit, and every tracked feature that does not follow the result becomes (-1, -1, KLT_MODEL_OUTLIER, aux).
 * It reads two feature lists and nothing else (no frame), and runs stream-ordered behind whatever wrote them.
 *
 * THE RULE.  Inputs: lists `in` and `out` of n records (the tracker's input and its result) and klt_model_params.  All arithmetic is
 * FP64, one rounding per operation, nothing contracted, in exactly the order written here; the device code divides nothing and takes
 * no square root: a model is kept in homogeneous form, six numerators and one denominator, q = (N / D) (p, 1).
 * Magnitudes: coordinates are below 2^16 and n below 2^24, so a hypothesis's numbers stay below 2^34, its residuals' squares below
 * 2^106, the refit's sums below 2^56, its cofactors below 2^114, its numerators and determinant below 2^172 and the squares of the
 * residuals under it below 2^380 -- nothing comes near 2^1023, nothing overflows.
 *  1 candidates  record i is a candidate iff in.val >= 0, out.val == KLT_TRACKED and all four coordinates satisfy 0 <= x < ncols,
 *                0 <= y < nrows as f32 comparisons (NaN and the infinities fail; a slot a replacement pass refilled, val > 0, is not
 *                one).  Candidates are numbered k = 0 .. m-1 in list order; p_k = ((double)in.x - cx, (double)in.y - cy), q_k likewise
 *                from out, cx = ncols / 2, cy = nrows / 2 (integer division).  m < min_inliers: no model (valid = 0), out untouched.
 *  2 samples     hypothesis h = 0 .. hypotheses-1 takes candidates r_j = mulhi32(mix(seed ^ mix(3*h + j)), m), j = 0, 1, 2, in uint32
 *                arithmetic: mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;
 *                mulhi32(u, m) = (uint64)u * m >> 32.  Repeated or collinear picks need no special case: their area is 0.
 *  3 hypothesis  with p0 = p_r0 ..., u = p1 - p0, v = p2 - p0, a = q1 - q0, b = q2 - q0 (componentwise):
 *                  D   = u.x*v.y - u.y*v.x
 *                  Nxx = a.x*v.y - b.x*u.y      Nxy = b.x*u.x - a.x*v.x      Ntx = D*q0.x - (Nxx*p0.x + Nxy*p0.y)
 *                  Nyx = a.y*v.y - b.y*u.y      Nyy = b.y*u.x - a.y*v.x      Nty = D*q0.y - (Nyx*p0.x + Nyy*p0.y)
 *                It counts iff fabs(D) >= (double)min_area (NaN fails); otherwise its score is -1.  Candidate k is an inlier of a
 *                model (N, D) iff rx*rx + ry*ry <= (t*t) * (D*D) with t = (double)max_error,
 *                  rx = ((Nxx*p.x + Nxy*p.y) + Ntx) - D*q.x        ry = ((Nyx*p.x + Nyy*p.y) + Nty) - D*q.y
 *                The score is the number of inliers.  The best hypothesis has the largest score, ties go to the smallest h.  Best
 *                score < min_inliers: valid = 0, out untouched.
 *  4 refit, once over the inliers of the best hypothesis, twelve sums: S1 = SUM 1.0, Sx = SUM p.x, Sy = SUM p.y, Sxx = SUM p.x*p.x,
 *                Sxy = SUM p.x*p.y, Syy = SUM p.y*p.y and, for the right-hand sides, X0 = SUM p.x*q.x, X1 = SUM p.y*q.x, X2 = SUM q.x,
 *                Y0 = SUM p.x*q.y, Y1 = SUM p.y*q.y, Y2 = SUM q.y.  The term of candidate k joins partial k mod 64 in increasing k
 *                (non-inliers are skipped), the 64 partials fold by p[l] += p[l + w], l < w, w = 32 .. 1.  Cramer's rule on the 3x3
 *                normal equations, through the cofactors
 *                  c00 = Syy*S1 - Sy*Sy      c01 = Sx*Sy - Sxy*S1      c02 = Sxy*Sy - Sx*Syy
 *                  c11 = Sxx*S1 - Sx*Sx      c12 = Sxy*Sx - Sxx*Sy     c22 = Sxx*Syy - Sxy*Sxy
 *                  D2  = (Sxx*c00 + Sxy*c01) + Sx*c02
 *                  Nxx = (c00*X0 + c01*X1) + c02*X2    Nxy = (c01*X0 + c11*X1) + c12*X2    Ntx = (c02*X0 + c12*X1) + c22*X2
 *                  Nyx, Nyy, Nty likewise from Y0, Y1, Y2.
 *                D2 > 0 (NaN fails): the model is the refit with D = D2, valid = 1.  Otherwise the hypothesis is kept, valid = 2.  The
 *                inlier test of step 3 is evaluated once more under the final model; there is no iteration.
 *  5 outputs     every candidate that is not an inlier of the final model becomes (-1, -1, KLT_MODEL_OUTLIER, out.aux) in `out`; every
 *                other record of `out` keeps its bytes.  One klt_motion_model goes to a feature buffer of five klt_feat records:
 *                valid = 0: the seven numbers, n_inliers and hypothesis_inliers are 0, hypothesis is -1; otherwise the final model,
 *                its inlier count, the best hypothesis and its score.  n_candidates = m; pad = ncols | nrows << 16 in every record the
 *                check writes (what klt_motion_model_affine uncentres with).  The division happens on the host. */
typedef struct { int32_t mode; int32_t ncols, nrows; int32_t hypotheses; uint32_t seed; int32_t min_inliers; float max_error; float min_area; } klt_model_params;
typedef struct { double nxx, nxy, ntx, nyx, nyy, nty, d; int32_t valid, n_candidates, n_inliers, hypothesis, hypothesis_inliers, pad; } klt_motion_model;
/* mode: 0 = off (the default), 1 = affine; anything else is KLT_ERR_ARG, and so are hypotheses outside 1 .. 65536, min_inliers < 3,
 * max_error or min_area negative or NaN, and (mode 1) ncols / nrows outside 1 .. 65535.  Defaults: 256 hypotheses, seed 0, min_inliers 8,
 * max_error 1.0 px, min_area 1.0 px^2.  Not in the reference; DESIGN.md section 9g. */
int klt_set_model_params(klt_ctx *ctx, const klt_model_params *p);
/* The check on two resident lists: fb_out is rewritten in place, fb_model (allocated if needed) takes the klt_motion_model; fb_model
 * must be distinct from fb_in and fb_out by index and by address, and fb_in from fb_out (KLT_ERR_ARG); lists shorter than n:
 * KLT_ERR_STATE; mode 0: KLT_ERR_STATE with a klt_last_error text; n == 0: KLT_OK, nothing enqueued.  The candidate and score scratch
 * belongs to the context (out of memory: KLT_ERR_NOMEM, nothing half-allocated).  Not in the reference; DESIGN.md section 9g. */
int klt_motion_check_async(klt_ctx *ctx, int fb_in, int fb_out, int fb_model, int n);
/* npairs pairs in the same launches; every fb_model distinct from every list and from each other, every fb_out from every other list.
 * Not in the reference; DESIGN.md section 9g. */
int klt_motion_check_batch_async(klt_ctx *ctx, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n);
/* synchronous, host arrays: out is rewritten, *model filled, *n_outliers (may be NULL) = the records that became KLT_MODEL_OUTLIER.
 * Not in the reference; DESIGN.md section 9g. */
int klt_motion_check(klt_ctx *ctx, const klt_feat *in, klt_feat *out, klt_motion_model *model, int n, int *n_outliers);
/* host only: the map q = A p + t (A row-major) in UNCENTRED pixel coordinates from a model record; KLT_ERR_ARG for a null pointer,
 * KLT_ERR_STATE for a record with valid == 0 or d == 0.  Not in the reference; DESIGN.md section 9g. */
int klt_motion_model_affine(const klt_motion_model *model, double A[4], double t[2]);
/* 0: no motion-check launch yet; 1: the last one ran as three launches on one pair, 2: as three launches on a table of pairs.  A
 * diagnostic, like klt_track_light_path.  Not in the reference; DESIGN.md section 9g. */
int klt_motion_check_path(klt_ctx *ctx);

/* ---- epipolar check (not in the reference) ---------------------------------------------------------------------- */
/* The motion-model check's sibling for a camera that translates through a scene with depth, where parallax is no affine motion: a seeded
 * consensus search for the pair's fundamental matrix F (q^T F p = 0), one least-squares refit, and every tracked feature off the
 * result becomes (-1, -1, KLT_EPIPOLAR_OUTLIER, aux).  It reads two feature lists and nothing else, and runs stream-ordered behind
 * whatever wrote them.  Under pure rotation, a planar scene or an exact image translation F is not unique: the check then flags less,
 * never more, and the motion-model check is the tool.
 *
 * THE RULE.  Inputs: lists `in` and `out` of n records and klt_epipolar_params.  All arithmetic is FP64, one rounding per operation,
 * nothing contracted, in exactly the order written here; only +, -, * and comparisons: no division, no square root.
 * Magnitudes: working coordinates lie in [-1, 1] (step 1), so every entry of a row is at most 1 and the 45 sums stay below n < 2^24.
 * In null9 step k first scales the remaining block so that its largest entry, the pivot P, has 0.5 <= |P| < 1; the update
 * A[i][j]*P - A[k][j]*A[i][k] of entries below 1 then stays below 2, and the next step scales again: nothing grows from step to step.
 * In the back-substitution every |A[i][j]| <= |A[i][i]| < 1, so after row i the largest |x| is at most 9 times the previous one:
 * |x| < 9^8 < 2^26, and x[8] is a product of eight pivots, at least 2^-8: f never is all zero.  a and b of the inlier test are then
 * below 2^28, r*r and den below 2^60.  Nothing comes near 2^1023 or 2^-1022: nothing overflows, nothing that matters underflows.
 *  1 candidates  exactly step 1 of the motion-model rule (same conditions, list order, cx = ncols / 2, cy = nrows / 2).  With k the
 *                smallest integer with 2 * (1 << k) >= max(ncols, nrows) and s = 2^-k, the working coordinates are the centred ones
 *                times s (exact): p = (((double)in.x - cx) * s, ((double)in.y - cy) * s), q likewise from out.  m < min_inliers: no
 *                model (valid = 0), out untouched.
 *  2 samples     hypothesis h takes candidates r_j = mulhi32(mix(seed ^ mix(8*h + j)), m), j = 0 .. 7 (mix, mulhi32: the motion-model rule).
 *  3 row         of a correspondence: (q.x*p.x, q.x*p.y, q.x, q.y*p.x, q.y*p.y, q.y, p.x, p.y, 1.0), the coefficients of q^T F p for F
 *                row-major as f[0 .. 8].
 *  4 null9(A)    the null vector of an 8x9 matrix.  For k = 0 .. 7: the pivot is the entry of largest |value| in rows k .. 7, columns
 *                k .. 8, the bits of |value| compared as integers, ties to the smallest row, then the smallest column.  ef = its biased
 *                exponent field; ef == 0 or ef == 0x7ff (zero, subnormal, non-finite): null9 fails.  Otherwise rows k and the pivot's,
 *                then columns k and the pivot's, are swapped (the column permutation is remembered); every entry of rows k .. 7,
 *                columns k .. 8 is multiplied by the double whose bits are (2045 - ef) << 52, a power of two that leaves the pivot P
 *                with 0.5 <= |P| < 1; and for rows i > k, columns j > k: A[i][j] = A[i][j]*P - A[k][j]*A[i][k], two products and one
 *                difference.  Back-substitution: x[8] = 1; for i = 7 .. 0: sum = ((A[i][i+1]*x[i+1] + A[i][i+2]*x[i+2]) + ...) left
 *                to right, then x[j] = x[j]*A[i][i] for every j > i, then x[i] = -sum.  Last the column permutation is undone.  Two
 *                equal rows leave an exactly zero row: repeated picks need no special case.
 *  5 hypothesis  f = null9 of the eight rows of its picks; null9 fails: score -1.  Candidate k is an inlier of f iff r*r <= t2 * den
 *                (NaN fails), the Sampson distance cross-multiplied, with t2 = ts*ts, ts = (double)max_error * s and
 *                  a0 = (f0*p.x + f1*p.y) + f2    a1 = (f3*p.x + f4*p.y) + f5    a2 = (f6*p.x + f7*p.y) + f8
 *                  b0 = (f0*q.x + f3*q.y) + f6    b1 = (f1*q.x + f4*q.y) + f7
 *                  r  = (a0*q.x + a1*q.y) + a2    den = ((a0*a0 + a1*a1) + b0*b0) + b1*b1
 *                The score is the number of inliers; the best hypothesis has the largest score, ties go to the smallest h.  Best
 *                score < min_inliers: valid = 0, out untouched.
 *  6 refit, once the 45 sums M[i][j] = SUM row[i]*row[j], i <= j, over the inliers of the best hypothesis (M is symmetric): the term of
 *                candidate k joins partial k mod 64 in increasing k (non-inliers are skipped), the 64 partials fold by
 *                p[l] += p[l + w], l < w, w = 32 .. 1.  g = the index of the largest |f_i| of the hypothesis, ties to the smallest.
 *                f' = null9(M without row g): the normal equations of least squares with f_g free.  null9 succeeds: the model is f',
 *                valid = 1; otherwise the hypothesis is kept, valid = 2.  The inlier test is evaluated once more under the final
 *                model; there is no iteration.
 *  7 outputs     every candidate that is not an inlier of the final model becomes (-1, -1, KLT_EPIPOLAR_OUTLIER, out.aux) in `out`;
 *                every other byte of `out` stays.  One klt_epipolar_model goes to a feature buffer of six klt_feat records: valid = 0:
 *                f, n_inliers and hypothesis_inliers are 0, hypothesis is -1; otherwise the final model (in working coordinates), its
 *                inlier count, the best hypothesis and its score.  n_candidates = m; pad = ncols | nrows << 16 in every record. */
typedef struct { int32_t mode; int32_t ncols, nrows; int32_t hypotheses; uint32_t seed; int32_t min_inliers; float max_error; } klt_epipolar_params;
typedef struct { double f[9]; int32_t valid, n_candidates, n_inliers, hypothesis, hypothesis_inliers, pad; } klt_epipolar_model;
/* mode: 0 = off (the default), 1 = on; anything else is KLT_ERR_ARG, and so are hypotheses outside 1 .. 65536, min_inliers < 8,
 * max_error negative or NaN, and (mode 1) ncols / nrows outside 1 .. 65535.  Defaults: 512 hypotheses, seed 0, min_inliers 16,
 * max_error 1.0 px.  Not in the reference; DESIGN.md section 9h. */
int klt_set_epipolar_params(klt_ctx *ctx, const klt_epipolar_params *p);
/* The check on two resident lists, with the conventions of klt_motion_check_async: fb_out is rewritten in place, fb_model (allocated if
 * needed, six records) takes the klt_epipolar_model; the three buffers pairwise distinct by index and by address (KLT_ERR_ARG); lists
 * shorter than n: KLT_ERR_STATE; mode 0: KLT_ERR_STATE with a klt_last_error text; n == 0: KLT_OK, nothing enqueued.  The scratch
 * belongs to the context and to this check alone (out of memory: KLT_ERR_NOMEM, nothing half-allocated). */
int klt_epipolar_check_async(klt_ctx *ctx, int fb_in, int fb_out, int fb_model, int n);
/* npairs pairs in the same launches; every fb_model distinct from every list and from each other, every fb_out from every other list. */
int klt_epipolar_check_batch_async(klt_ctx *ctx, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n);
/* synchronous, host arrays: out is rewritten, *model filled, *n_outliers (may be NULL) = the records that became KLT_EPIPOLAR_OUTLIER. */
int klt_epipolar_check(klt_ctx *ctx, const klt_feat *in, klt_feat *out, klt_epipolar_model *model, int n, int *n_outliers);
/* host only: F (row-major) in UNCENTRED pixel coordinates, q^T F p = 0 for p in frame 1 and q in frame 2: T^T f T with
 * T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], scaled to unit Frobenius norm.  KLT_ERR_ARG for a null pointer, KLT_ERR_STATE for a
 * record with valid == 0 (or one whose norm is zero or not finite). */
int klt_epipolar_matrix(const klt_epipolar_model *model, double F[9]);
/* 0: no epipolar-check launch yet; 1: the last one ran as three launches on one pair, 2: on a table of pairs.  A diagnostic. */
int klt_epipolar_check_path(klt_ctx *ctx);

/* ---- homography check (not in the reference) -------------------------------------------------------------------- */
/* The third consensus check, for a camera that ROTATES (pan / tilt, hand-held) and for any camera that looks at a PLANE (aerial nadir
 * view, road surface, document, wall): the static scene then moves by a homography q ~ H p, whose perspective part an affine map cannot
 * follow and for which the fundamental matrix is not unique.  A seeded consensus search over four-point hypotheses finds the pair's
 * homography, one least-squares refit, and every tracked feature off the result becomes (-1, -1, KLT_HOMOGRAPHY_OUTLIER, aux).  It reads
 * two feature lists and nothing else, and runs stream-ordered behind whatever wrote them.  Limits: exactly collinear correspondences
 * fit a family of homographies: the check then flags less, never more; candidates that lie NEARLY on one line with noise on them make
 * every four-point hypothesis ill-conditioned, and good tracks are flagged: the check wants candidates spread
 * over the frame in both directions.  A scene with parallax (a camera that translates through depth) is NOT a homography: the check
 * then flags most of the static tracks, and the epipolar check is the tool.
 *
 * THE RULE.  Inputs: lists `in` and `out` of n records and klt_homography_params.  All arithmetic is FP64, one rounding per operation,
 * nothing contracted, in exactly the order written here; only +, -, * and comparisons: no division, no square root.
 * Magnitudes: working coordinates lie in [-1, 1] (step 1), so every entry of a row is at most 1 in magnitude; a term of the 24 sums is at
 * most 2 (q.x*q.x + q.y*q.y) and the sums stay below 2 n < 2^26.  null9's bounds are those of the epipolar rule, unchanged: the remaining
 * block is rescaled in every step, |x| < 9^8 < 2^26 and h never is all zero.  u, v and w of the inlier test are then below 3 * 2^26 < 2^28,
 * w*q.x likewise, rx and ry below 2^29 and every square and their sum below 2^60.  Nothing comes near 2^1023 or 2^-1022.
 *  1 candidates  exactly step 1 of the epipolar rule: the same conditions, list order, cx = ncols / 2, cy = nrows / 2, s = 2^-k with k the
 *                smallest integer with 2 * (1 << k) >= max(ncols, nrows); p = (((double)in.x - cx) * s, ((double)in.y - cy) * s), q
 *                likewise from out.  m < min_inliers: no model (valid = 0), out untouched.
 *  2 samples     hypothesis h takes candidates r_j = mulhi32(mix(seed ^ mix(4*h + j)), m), j = 0 .. 3 (mix, mulhi32: the motion-model rule).
 *  3 rows        correspondence j gives rows 2j and 2j+1 of the 8x9 matrix, the coefficients of h[0 .. 8] (H row-major):
 *                  (p.x, p.y, 1.0, 0.0, 0.0, 0.0, -(q.x*p.x), -(q.x*p.y), -q.x)
 *                  (0.0, 0.0, 0.0, p.x, p.y, 1.0, -(q.y*p.x), -(q.y*p.y), -q.y)
 *                one product, then its negation (exact); the zeros are +0.0.
 *  4 null9(A)    step 4 of the epipolar rule, bit for bit.  Repeated picks leave exactly zero rows: null9 fails, no special case.
 *  5 hypothesis  h = null9 of the eight rows of its picks; null9 fails: score -1.  With
 *                  u = (h0*p.x + h1*p.y) + h2    v = (h3*p.x + h4*p.y) + h5    w = (h6*p.x + h7*p.y) + h8
 *                  rx = u - w*q.x                ry = v - w*q.y
 *                candidate k is an inlier of h iff rx*rx + ry*ry <= t2 * (w*w) (NaN fails), the forward transfer error
 *                cross-multiplied, with t2 = ts*ts, ts = (double)max_error * s.  The score is the number of inliers; the best
 *                hypothesis has the largest score, ties go to the smallest h.  Best score < min_inliers: valid = 0, out untouched.
 *  6 refit, once least squares on the same rows over the inliers of the best hypothesis.  With e = (p.x, p.y, 1.0) the normal matrix is
 *                M = [[A, 0, -Bx], [0, A, -By], [-Bx, -By, C]], 3x3 symmetric blocks, 24 sums over (i, j), i <= j:
 *                  A[i][j] = SUM ee    Bx[i][j] = SUM q.x*ee    By[i][j] = SUM q.y*ee    C[i][j] = SUM qq*ee
 *                with ee = e_i*e_j (one product; a factor 1.0 is exact) and qq = q.x*q.x + q.y*q.y (two products, one sum).  The term
 *                of candidate k joins partial k mod 64 in increasing k (non-inliers are skipped), the 64 partials fold by
 *                p[l] += p[l + w], l < w, w = 32 .. 1.  The blocks are mirrored, -Bx and -By are the negated sums, the structural zeros
 *                are +0.0.  g = the index of the largest |h_i| of the hypothesis, ties to the smallest.  h' = null9(M without row g).
 *                null9 succeeds: the model is h', valid = 1; otherwise the hypothesis is kept, valid = 2.  The inlier test is evaluated
 *                once more under the final model; there is no iteration.
 *  7 outputs     every candidate that is not an inlier of the final model becomes (-1, -1, KLT_HOMOGRAPHY_OUTLIER, out.aux) in `out`;
 *                every other byte of `out` stays.  One klt_homography_model goes to a feature buffer of six klt_feat records: valid = 0:
 *                h, n_inliers and hypothesis_inliers are 0, hypothesis is -1; otherwise the final model (in working coordinates), its
 *                inlier count, the best hypothesis and its score.  n_candidates = m; pad = ncols | nrows << 16 in every record. */
typedef struct { int32_t mode; int32_t ncols, nrows; int32_t hypotheses; uint32_t seed; int32_t min_inliers; float max_error; } klt_homography_params;
typedef struct { double h[9]; int32_t valid, n_candidates, n_inliers, hypothesis, hypothesis_inliers, pad; } klt_homography_model;
/* mode: 0 = off (the default), 1 = on; anything else is KLT_ERR_ARG, and so are hypotheses outside 1 .. 65536, min_inliers < 4,
 * max_error negative or NaN, and (mode 1) ncols / nrows outside 1 .. 65535.  Defaults: 256 hypotheses, seed 0, min_inliers 8,
 * max_error 1.0 px.  Not in the reference; DESIGN.md section 9i. */
int klt_set_homography_params(klt_ctx *ctx, const klt_homography_params *p);
/* The check on two resident lists, with the conventions and refusals of klt_epipolar_check_async: fb_out is rewritten in place, fb_model
 * (allocated if needed, six records) takes the klt_homography_model.  The scratch belongs to the context and to this check alone: all
 * three consensus checks may be on in one context. */
int klt_homography_check_async(klt_ctx *ctx, int fb_in, int fb_out, int fb_model, int n);
/* npairs pairs in the same launches; every fb_model distinct from every list and from each other, every fb_out from every other list. */
int klt_homography_check_batch_async(klt_ctx *ctx, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n);
/* synchronous, host arrays: out is rewritten, *model filled, *n_outliers (may be NULL) = the records that became KLT_HOMOGRAPHY_OUTLIER. */
int klt_homography_check(klt_ctx *ctx, const klt_feat *in, klt_feat *out, klt_homography_model *model, int n, int *n_outliers);
/* host only: H (row-major) in UNCENTRED pixel coordinates, q ~ H p for p in frame 1 and q in frame 2: T^-1 h T with
 * T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]] (T^-1 holds 2^k: exact), scaled to unit Frobenius norm, with the sign that makes the
 * third coordinate positive at the image centre (working h[8] > 0).  KLT_ERR_ARG for a null pointer, KLT_ERR_STATE for a record with
 * valid == 0 (or one whose norm is zero or not finite). */
int klt_homography_matrix(const klt_homography_model *model, double H[9]);
/* 0: no homography-check launch yet; 1: the last one ran as three launches on one pair, 2: on a table of pairs.  A diagnostic. */
int klt_homography_check_path(klt_ctx *ctx);

/* ---- crowding check (not in the reference) ----------------------------------------------------------------------- */
/* Selection keeps features mindist apart and the replacement pass keeps every NEW feature mindist away from the live ones; nothing keeps
 * the live ones apart once they move (a zoom-out, a camera that backs away, two tracks that slide onto one corner).  This check drops
 * every tracked feature that has come within min_distance of an older one: the missing half of that invariant.  It reads one feature
 * list (and the previous step's crowd records) and no frame, and runs stream-ordered behind whatever wrote them.
 *
 * THE RULE (serial; the device equals it byte for byte).  Inputs: a list `out` of n records, optionally n klt_crowd records `prev` (the
 * previous step's output), ncols, nrows and min_distance d >= 1; r = d - 1, as the minimum-distance walk of selection works with
 * mindist - 1.
 *  1 candidates  record i is a candidate iff out.val == KLT_TRACKED, 0 <= x < ncols and 0 <= y < nrows: f32 comparisons (NaN and the
 *                infinities fail; -0.0 passes), made before any conversion.  Its pixel is px = (int)x, py = (int)y, by truncation, as
 *                the reference's int(feat.x) when it stamps the live features into its feature map.
 *  2 age in      a_i = max(prev[i].age, 0); without prev every a_i is 0.
 *  3 order       candidates are ordered by age descending, then by list index ascending.
 *  4 walk        in that order candidate i is CROWDED iff an earlier KEPT candidate j has |px_i - px_j| <= r and |py_i - py_j| <= r;
 *                otherwise it is kept.  This is the reference's feature map: offered the candidates' pixels as a point list in this
 *                order, its walk accepts exactly the kept ones.  The WINNER of a crowded candidate is the first kept candidate in the
 *                order that covers it.
 *  5 outputs     crowded records of `out` become (-1, -1, KLT_CROWDED, out.aux); every other record of `out` keeps its bytes.  One
 *                klt_crowd is written per record: kept (min(a_i, INT32_MAX - 1) + 1, -1, 1, 0); crowded (0, winner's index, 2, 0);
 *                non-candidate (0, -1, 0, 0).
 * `age` so counts the consecutive steps a slot has been tracked: a slot that was lost, flagged by any check or refilled by the
 * replacement pass starts again at 0; `winner` tells which track a dropped one merged into.  The crowd records go to a buffer of their
 * own and nothing but `out` is updated in place: a step may be enqueued ahead and repeated, like the stateless tracker launches.
 * Afterwards no two live records are within r px of each other (Chebyshev distance on integer pixels): what the replacement pass
 * assumes of the list it stamps.
 * The device finds the same set in rounds -- kept, if every higher-priority neighbour is crowded; crowded, if any is kept -- inside ONE
 * workgroup per list (no workgroup ever waits for another); the number of rounds depends on the data (a chain of k candidates spaced r
 * apart with falling ages takes k), the loop ends when no candidate is undecided. */
typedef struct { int32_t mode; int32_t ncols, nrows; int32_t min_distance; } klt_crowd_params;
typedef struct { int32_t age, winner, val, pad; } klt_crowd;     /* val: 0 non-candidate, 1 kept, 2 crowded */
/* mode: 0 = off (the default), 1 = on; anything else is KLT_ERR_ARG, and so are min_distance < 1 and (mode 1) ncols / nrows outside 1 .. 65535. */
int klt_set_crowd_params(klt_ctx *ctx, const klt_crowd_params *p);
/* The check on a resident list: fb_out is rewritten in place, fb_prev (-1: none) holds the previous step's klt_crowd records, fb_crowd
 * (allocated if needed; klt_crowd records live in feature buffers as klt_quality records do) takes this step's.  fb_crowd must be
 * distinct from fb_out and fb_prev, by index and by address (KLT_ERR_ARG); lists shorter than n: KLT_ERR_STATE; mode 0: KLT_ERR_STATE
 * with a klt_last_error text; n == 0: KLT_OK, nothing is enqueued.  Three launches, no host synchronisation; the scratch belongs to the
 * context (KLT_ERR_NOMEM when it cannot grow, the context stays usable). */
int klt_crowd_check_async(klt_ctx *ctx, int fb_out, int fb_prev, int fb_crowd, int n);
/* npairs lists in the same three launches (fb_prev may be NULL: none has a previous step; or hold -1 entries); every fb_crowd distinct
 * from every other buffer of the call, every fb_out from every other fb_out. */
int klt_crowd_check_batch_async(klt_ctx *ctx, const int *fb_out, const int *fb_prev, const int *fb_crowd, int npairs, int n);
/* synchronous, host arrays: out is rewritten, crowd filled, *n_crowded (may be NULL) = the records that became KLT_CROWDED. */
int klt_crowd_check(klt_ctx *ctx, klt_feat *out, const klt_crowd *prev, klt_crowd *crowd, int n, int *n_crowded);
/* 0: no crowd-check launch yet; 1: the last one ran on one list, 2: on a table of lists.  A diagnostic. */
int klt_crowd_check_path(klt_ctx *ctx);
/* The rounds the last single-list launch took (the first list's of a batch), read back from the device: synchronises.  phase_ticks (may
 * be NULL) takes what the resolve launch's one workgroup spent grouping the candidates by cell, in the rounds and writing the records,
 * in ticks of 10 ns.  A diagnostic; KLT_ERR_STATE before any crowd-check launch. */
int klt_crowd_check_rounds(klt_ctx *ctx, int *rounds, int *phase_ticks);

/* ---- CLAHE ingest stage (not in the reference) ------------------------------------------------------------------- */
/* Contrast-limited adaptive histogram equalisation of an 8-bit frame in front of the level-0 kernel: in a low-contrast frame (a dark
 * half, a backlit scene, a thermal camera squeezed into 8 bits) the 7x7 sums of the selection sit in a few grey levels and min_eigenvalue
 * turns away corners a person would pick.  With mode 1 every reader of a slot's raw 8-bit frame -- the level-0 launch of a build, the
 * two-pass build, the selection on the raw frame (use_pyramid = 0) -- reads an equalised copy the slot keeps instead; the frame itself
 * (an adopted frame is the caller's memory) is read and never written.
 *
 * THE RULE (integer arithmetic only; the device equals it byte for byte).  Inputs: an 8-bit frame ncols x nrows, tiles_x, tiles_y, clip_q8
 * (the clip limit times 256, rounded; 0 = no clipping).
 *  1 tiles     edges x_k = (k * ncols) / tiles_x, k = 0 .. tiles_x, and y_j likewise (integer division): tiles differ by at most one pixel
 *              in size, nothing is padded.
 *  2 per tile  (area A, 256-bin histogram h)  if clip_q8 > 0: cap = max(1, (clip_q8 * A) >> 16) in 64 bits; excess = SUM max(h[b] - cap, 0);
 *              h[b] = min(h[b], cap) + excess / 256; with r = excess % 256 the bins (k * 256) / r, k = 0 .. r - 1, get one more each.  No
 *              second clipping pass; the bins still sum to A.  cdf[b] = the inclusive prefix sum of h; lut[b] = (cdf[b] * 255 + A / 2) / A.
 *  3 per axis  in doubled coordinates, C_k = x_k + x_{k+1} and P = 2 x + 1:  P < C_0: both tiles 0, w = 0, D = 1;  P >= C_{tiles_x - 1}:
 *              both tiles tiles_x - 1, w = 0, D = 1;  otherwise with k the largest value with C_k <= P: tiles k and k + 1, w = P - C_k,
 *              D = C_{k+1} - C_k.  (One tile on an axis: D is always 1.)
 *  4 pixel     with v the input byte: (lut00[v] (Dx - wx) (Dy - wy) + lut10[v] wx (Dy - wy) + lut01[v] (Dx - wx) wy + lut11[v] wx wy
 *              + (Dx Dy) / 2) / (Dx Dy): one rounding, 0 .. 255 (lut10: the tile one to the right, lut01: the tile one down).
 * A frame is EQUALISABLE when tiles_x <= ncols, tiles_y <= nrows and the largest Dx * Dy * 255 is below 2^32 (the per-pixel division is a
 * 32-bit one; at 3840 x 2160 this holds from 2 x 2 tiles up, and for 1 x 1); otherwise KLT_ERR_ARG, and the slot stays usable.
 * Two launches per build (per-tile LUTs; the interpolated frame), the frames of a build's group in the same two. */
typedef struct { int32_t mode; int32_t tiles_x, tiles_y; int32_t clip_q8; } klt_equalize_params;
/* mode: 0 = off (the default), 1 = CLAHE; tiles_x, tiles_y in 1 .. 64; clip_q8 in 0 .. 2^20; anything else is KLT_ERR_ARG.  A change
 * voids every slot's equalised frame and counts as a change of the taps does: every slot's next build is a full one, lean slots included.
 * The pyramids a slot holds stay what their build made them (klt_slot_state keeps saying so): the caller rebuilds. */
int klt_set_equalize_params(klt_ctx *ctx, const klt_equalize_params *p);
/* A host frame (pitch bytes from row to row) in, the equalised host frame (ncols bytes from row to row) out, like klt_smooth_f32: the
 * two kernels by name, under the context's tiles and clip limit whatever its mode says.  Synchronises.  A frame that is not equalisable:
 * KLT_ERR_ARG. */
int klt_equalize_u8(klt_ctx *ctx, const uint8_t *src, int ncols, int nrows, int pitch, uint8_t *dst);
/* The equalised frame the slot's last build (or selection on the raw frame) read, [nrows][ncols] bytes: KLT_ERR_STATE if that was not an
 * equalised one -- mode 0, or a new frame or new parameters since.  Synchronises. */
int klt_download_equalized_u8(klt_ctx *ctx, int slot, uint8_t *dst);
/* 0: the last klt_build_pyramids* enqueued no equalisation launch (mode 0, or every slot's equalised frame was still valid), 1: it did.
 * A diagnostic, like klt_track_light_path. */
int klt_equalize_path(klt_ctx *ctx);
/* With mode 1, klt_build_pyramids* and the selection on the raw frame refuse an f32 slot: KLT_ERR_STATE, "equalisation takes 8-bit
 * frames"; nothing is enqueued and the slot builds again with mode 0.  The slot's equalised frame lives in a buffer of its own, allocated
 * when first needed (KLT_ERR_NOMEM leaves the slot as it was), freed by klt_slot_free, travelling with klt_swap_slots.  With mode 0 no
 * launch, no allocation and no event is added to any call. */

/* ---- Remap ingest stage (not in the reference) -------------------------------------------------------------------- */
/* A fixed-point remap with bilinear interpolation of an 8-bit frame in front of the level-0 kernel -- lens undistortion, stereo
 * rectification, fisheye to pinhole, a rotated camera mount: the epipolar and the homography check assume a pinhole camera, and on a
 * wide-angle lens they flag good tracks toward the frame's edges.  With a map set every reader of a slot's raw 8-bit frame -- the level-0
 * launch of a build, the two-pass build, the selection on the raw frame (use_pyramid = 0), the CLAHE stage -- reads a remapped copy the
 * slot keeps instead; the frame itself (an adopted frame is the caller's memory) is read and never written.  With both ingest stages on
 * the order is remap, then CLAHE.
 *
 * THE RULE (integer arithmetic only; the device equals it byte for byte).  Inputs: an 8-bit source frame ncols x nrows; a map of the
 * same ncols x nrows that holds for each destination pixel two int32 values mx, my: the source position in 1/256 px, pixel centres at
 * integers (KLT's coordinates).  Any int32 value is legal.
 *  1 clamp     X = min(max(mx, 0), (ncols - 1) * 256), Y = min(max(my, 0), (nrows - 1) * 256): edge replication, not a fill colour (a
 *              fill would draw a curved black border that the selection takes for corners).
 *  2 split     x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, ncols - 1); y0, fy, y1 likewise.
 *  3 pixel     out = ((256 - fx) (256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16 in unsigned 32 bits,
 *              p10 the pixel at (x1, y0), p01 at (x0, y1).  The largest sum is 65536 * 255 + 32768; the weights sum to 65536, so a
 *              constant frame stays constant under every map.
 * The destination has the shape of the source (a map that changes the frame size is not offered).  The clamp is done on the device for
 * every entry: no map content makes a read outside the source rows.  One launch per build, the frames of the build in it. */
/* The context's one map: two planes of ncols * nrows int32 (row-major, ncols entries from row to row), copied to the device before the
 * call returns.  NULL, NULL switches the stage off (the default; the sizes are then not looked at); one NULL, or a size outside
 * 1 .. 65535, is KLT_ERR_ARG.  A new map -- also the same values again -- or none voids every slot's remapped and equalised frame and
 * counts as a change of the taps does: every slot's next build is a full one.  The pyramids a slot holds stay what their build made
 * them: the caller rebuilds.  Synchronises. */
int klt_set_remap(klt_ctx *ctx, const int32_t *map_x, const int32_t *map_y, int ncols, int nrows);
/* A host frame (pitch bytes from row to row) in, the remapped host frame (ncols bytes from row to row) out: the kernel by name under
 * the context's map, whatever else is set.  Synchronises.  No map set: KLT_ERR_STATE; a size that is not the map's: KLT_ERR_ARG. */
int klt_remap_u8(klt_ctx *ctx, const uint8_t *src, int ncols, int nrows, int pitch, uint8_t *dst);
/* The remapped frame the slot's last build (or selection on the raw frame) read, [nrows][ncols] bytes: KLT_ERR_STATE if that was not a
 * remapped one -- no map set, or a new frame or a new map since.  Synchronises. */
int klt_download_remapped_u8(klt_ctx *ctx, int slot, uint8_t *dst);
/* 0: the last klt_build_pyramids* enqueued no remap launch (no map set, or every slot's remapped frame was still valid), 1: it did. */
int klt_remap_path(klt_ctx *ctx);
/* With a map set, klt_build_pyramids* and the selection on the raw frame refuse an f32 slot (KLT_ERR_STATE, "remapping takes 8-bit
 * frames") and a slot whose frame is not of the map's size (KLT_ERR_ARG, naming both sizes); nothing is enqueued, and the slot builds
 * again with no map or a fitting one.  The slot's remapped frame lives in a buffer of its own, allocated when first needed (KLT_ERR_NOMEM
 * leaves the slot as it was), freed by klt_slot_free, travelling with klt_swap_slots.  With no map set no launch, no allocation and no
 * event is added to any call. */

/* ---- descriptors (not in the reference) --------------------------------------------------------------------------- */
/* A 256-bit binary descriptor per feature from the 8-bit frame a slot holds, and a brute-force Hamming matcher over two descriptor sets:
 * what gives a feature an identity that survives a gap (an occlusion, a second camera, a revisited place).  Both rules are integer-only;
 * the device output equals their numpy restatement (tests/describe_expected.py) byte for byte.
 *
 * RULE 1, THE DESCRIPTOR.  Inputs: F, the ncols x nrows 8-bit frame that is the output of the slot's ingest chain (remapped, then
 * equalised, when those stages are on); a list of klt_feat; mode: 1 upright, 2 steered.
 *   1. centre    a feature is DESCRIBABLE when val >= 0, x and y are finite and, with cx = floor((double)x + 0.5), cy likewise,
 *                0 <= cx < ncols and 0 <= cy < nrows.  Every other record is all zero (val = 0).
 *   2. pixels    P(u, v) = F[clamp(cy + v, 0, nrows - 1)][clamp(cx + u, 0, ncols - 1)]: edges are replicated, as in the remap stage, so
 *                every describable feature gets a descriptor on any frame size, 1 x 1 included.
 *   3. pattern   256 tests (ax, ay, bx, by), generated once on the host and never typed in: state s = 0x9E3779B9 (uint32); a draw is
 *                s = s * 1664525 + 1013904223 (mod 2^32) with value ((s >> 16) % 27) - 13; draw ax, ay, bx, by in that order; discard
 *                the four if ax^2 + ay^2 > 169, or bx^2 + by^2 > 169, or (ax, ay) == (bx, by), or the test or its swap (bx, by, ax, ay)
 *                is in the list already; stop at 256 tests (1892 draws).
 *   4. orientation (mode 2; mode 1 has k = 0)  m10 = SUM u P(u, v), m01 = SUM v P(u, v) over u^2 + v^2 <= 225, 64-bit integers; k is the
 *                smallest index in 0 .. 31 that maximises m10 C[k] + m01 S[k], C[k] = round(16384 cos(2 pi k / 32)) =
 *                16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
 *                -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069
 *                and S[k] = C[(k + 24) % 32].  No libm call on either side of the comparison.
 *   5. steering  for k != 0 both points of every test are rotated: x' = (x C[k] - y S[k] + 8192) >> 14, y' = (x S[k] + y C[k] + 8192) >> 14,
 *                arithmetic shifts (floor).  No rotated coordinate exceeds 13 in magnitude: with the box of step 6 every read lies in
 *                the 31 x 31 patch around the centre, as does the orientation disc.
 *   6. bit       B(u, v) = the sum of P over the 5 x 5 box centred at (u, v) (at most 6375); bit t is 1 iff B(a'_t) < B(b'_t), and is
 *                bit t & 31 of bits[t >> 5].
 *   7. record    klt_descriptor, 48 bytes = three klt_feat records: val 1 described / 0 not; orientation = k; cx, cy the centre.  It
 *                lives in a feature buffer of 3 n records, the way quality and model records live in feature buffers.
 *
 * RULE 2, THE MATCH.  Inputs: nq query records, nt train records, klt_match_params.  Train record j is a CANDIDATE of query i when both
 * have val == 1 and, with radius > 0, |cx_i - cx_j| <= radius and |cy_i - cy_j| <= radius.  d(i, j) = popcount of the XOR of the 256
 * bits; best = the candidate of least d, a tie to the lowest j; second = the least d over the candidates other than best, 257 when there
 * is none.  The outcome, decided in the order of these val codes:
 *   0  the query is not described (train = -1, distance = second = 0);
 *   2  no candidate (train = -1, distance = second = 257);
 *   3  distance > max_distance;
 *   4  ratio on, and not distance * ratio_den < second * ratio_num (64-bit arithmetic, strict);
 *   5  cross-check on, and the best QUERY of train record `best` -- found by the same rule with the roles exchanged, ties to the lowest
 *      query index -- is not i;
 *   1  matched.
 * Codes 1, 3, 4 and 5 carry train = best and the two distances found.  One `struct klt_match` record (16 bytes, one klt_feat) per query. */
typedef struct { uint32_t bits[8]; int32_t val, orientation, cx, cy; } klt_descriptor;
typedef struct { int32_t mode; } klt_descriptor_params;                      /* 1 upright (default), 2 steered */
typedef struct { int32_t max_distance, ratio_num, ratio_den, cross_check, radius; } klt_match_params;
struct klt_match { int32_t train, distance, second, val; };      /* (a tag, not a typedef: klt_match is also the synchronous call) */
int klt_set_descriptor_params(klt_ctx *ctx, const klt_descriptor_params *p);      /* another mode: KLT_ERR_ARG */
/* Describes the n records of fb_in on the slot's 8-bit frame into fb_desc (3 n feature records, allocated if needed).  The frame is read
 * the way the selection on the raw frame reads it: behind its upload, behind a build that still reads it, through the ingest chain.  No
 * pyramid is needed.  Refused before anything is allocated or enqueued: a slot without a frame and an f32 slot ("descriptors take 8-bit
 * frames"): KLT_ERR_STATE; fb_desc the same buffer as fb_in, by index or by address, and n < 0: KLT_ERR_ARG; fb_in short of n records:
 * KLT_ERR_STATE.  n == 0: KLT_OK, nothing enqueued.  A failed allocation is KLT_ERR_NOMEM and the context stays usable. */
int klt_describe_async(klt_ctx *ctx, int slot, int fb_in, int fb_desc, int n);
int klt_describe(klt_ctx *ctx, int slot, const klt_feat *in, klt_descriptor *out, int n);      /* synchronous, host arrays */
/* max_distance 0 .. 256 (default 64); ratio_num == 0 switches the ratio test off, else 0 < ratio_num <= ratio_den <= 65535 (default
 * 4 / 5); cross_check 0 or 1 (default 1); radius >= 0, 0 = no gate (default).  Anything else: KLT_ERR_ARG. */
int klt_set_match_params(klt_ctx *ctx, const klt_match_params *p);
/* fb_query holds nq descriptors (3 nq feature records), fb_train nt; fb_match (nq feature records, allocated if needed) must be distinct
 * from both, by index and by address (KLT_ERR_ARG); fb_query may be fb_train.  nq == 0 enqueues nothing; nt == 0 gives every described
 * query val = 2.  The partial results of the train set's ranges go through scratch the context owns and grows (KLT_ERR_NOMEM). */
int klt_match_async(klt_ctx *ctx, int fb_query, int nq, int fb_train, int nt, int fb_match);
int klt_match(klt_ctx *ctx, const klt_descriptor *q, int nq, const klt_descriptor *t, int nt, struct klt_match *out);      /* synchronous, host arrays */
/* Diagnostic, read-only: *splits = how many ranges the train set of the last match was cut into (decided from nq and nt alone; every
 * cut gives the same records).  KLT_ERR_STATE before the first match. */
int klt_match_path(klt_ctx *ctx, int *splits);

/* ---- track identities (not in the reference) ----------------------------------------------------------------------- */
/* A persistent track id for every slot of every list of a sequence, and re-acquisition of lost tracks: what a lost track leaves behind
 * (descriptor, id, the step it was last seen) goes into a ring bank in device memory; every step the newly selected features are matched
 * against the bank (rule 2 above, cross-check always on) and inherit the old id on a match.  Everything is enqueued on the context's
 * stream; no call here synchronises except the three diagnostics.  Integer-only; the device output (ident rows, bank, state) equals
 * the numpy restatement (tests/reacquire_expected.py) byte for byte.
 *
 * STATE per context: the step counter k, next_id, the ring head h, a bank of C = capacity entries, the descriptors P of the previous list.
 *
 * BEGIN (list L0 of n records on the slot's frame):  I0[s] = {s, 0, 0, 2} where L0[s].val >= 0, else {-1, 0, 0, 0}; next_id = n, h = 0,
 * k = 0, every bank entry all zero; P = the descriptors of L0 (rule 1 in the context's descriptor mode).
 *
 * STEP k >= 1 (list Lk -- after tracking, checks and replacement --, the previous ident row I(k-1), frame k in the slot):
 *   1. Q = the descriptors of Lk on frame k.
 *   2. classes   slot s is CONTINUED when I(k-1)[s].val != 0 and Lk[s].val == 0; FRESH when Lk[s].val >= 0 and it is not continued; LOST
 *                when I(k-1)[s].val != 0 and it is not continued.  A refilled slot is both lost and fresh.
 *   3. expire    a valid bank entry with k - last_seen - 1 > max_gap becomes all zero.
 *   4. deposit   the lost slots with P[s].val == 1, in slot order, ranks r = 0 .. L-1: entry (h + r) & (C-1) = {P[s], I(k-1)[s].id,
 *                last_seen = k-1, valid = 1, pad = 0}; the outcome is that of writing all L in order (L > C: only ranks >= L - C are
 *                written); then h = (h + L) & (C-1).
 *   5. match     rule 2 with cross_check = 1: the queries are the C bank entries in position order (an entry that is not valid counts as
 *                not described), the train set is the fresh slots' Q records in slot order.
 *   6. assign    bank entry i with outcome 1 and train slot s: Ik[s] = {bank[i].id, k - bank[i].last_seen - 1, distance, 3}, and the
 *                entry becomes all zero.  The cross-check makes this conflict-free: entry i is matched only when the best query of its
 *                train record is i, and that is one value per train record.  The other fresh slots, in slot order with rank r:
 *                {next_id + r, 0, 0, 2}; next_id += their number.  Continued slots: {I(k-1)[s].id, 0, 0, 1}.  All others: {-1, 0, 0, 0}.
 *   7. P = Q.
 * Deposits come before the match: a track the tracker dropped and the replacement pass selected again in the same step gets its id back
 * with gap = 0. */
typedef struct { int32_t id, gap, distance, val; } klt_ident;      /* val: 0 no track (id = -1), 1 continued, 2 new, 3 re-acquired */
typedef struct { klt_descriptor d; int32_t id, last_seen, valid, pad; } klt_bank_entry;      /* 64 bytes */
typedef struct { int32_t capacity, max_gap, max_distance, ratio_num, ratio_den, radius; } klt_reacquire_params;
/* k, h and next_id after the last begin / step; the valid bank entries; the fresh slots and the deposited (lost and described) slots
 * of the last step */
struct klt_reacquire_state { int32_t k, h, next_id, valid, fresh, lost; };      /* (a tag, as klt_match is: the name is also the call) */
/* capacity a power of two in 1 .. 4096 (default 1024); max_gap >= 0 (default 30); max_distance, ratio_num, ratio_den, radius as
 * klt_set_match_params takes them (defaults 64, 4 / 5, 24).  Anything else: KLT_ERR_ARG.  New parameters end the sequence in progress:
 * the next call must be a begin. */
int klt_set_reacquire_params(klt_ctx *ctx, const klt_reacquire_params *p);
/* fb_list holds the n >= 1 records of the list, the slot its frame (read as klt_describe_async reads it, and refused as it refuses);
 * fb_ident (n feature records, allocated if needed) receives the klt_ident row.  Every refusal comes before the first allocation --
 * klt_describe_async's; fb_ident the same buffer as fb_list (or, in a step, fb_ident_prev), by index or by address, n < 1:
 * KLT_ERR_ARG; a step without a begin, with another n than the begin's, fb_ident_prev short of n records: KLT_ERR_STATE -- and every
 * allocation before the first launch; a failed one is KLT_ERR_NOMEM and the call can be repeated.  All memory is taken by the begin call:
 * a step allocates nothing, so steps may be captured into a graph. */
int klt_reacquire_begin_async(klt_ctx *ctx, int slot, int fb_list, int fb_ident, int n);
int klt_reacquire_step_async(klt_ctx *ctx, int slot, int fb_list, int fb_ident_prev, int fb_ident, int n);
/* Diagnostics.  The first two synchronise the context's stream; KLT_ERR_STATE before the first begin.  `entries` receives capacity
 * klt_bank_entry records.  klt_reacquire_path: *launches = the launches the last begin (2) or step (5) enqueued, 0 = none yet; a
 * context that never calls a begin makes exactly the calls it made before. */
int klt_reacquire_state(klt_ctx *ctx, struct klt_reacquire_state *state);
int klt_reacquire_download_bank(klt_ctx *ctx, void *entries);
int klt_reacquire_path(klt_ctx *ctx, int *launches);

/* ---- affine consistency check (BASELINE cfg-3) -- PARITY UNPINNED ------------------------- */
/* The reference calls _am_trackFeatureAffine / _am_getSubFloatImage at trackFeatures.py:347-399 but defines neither
 * (NameError): the call site pins the interface, upstream KLT 1.3.4 the behaviour.
 * mode = tc.affineConsistencyCheck (klt.py:67): -1 off, 0 translation, 1 similarity, 2 affine. */
typedef struct {
    int32_t mode, window_width, window_height, max_iterations;       /* klt.py:67-70 */
    float   max_residue, min_displacement, max_displacement_differ;   /* klt.py:71-73 */
} klt_affine_params;
/* per-feature state the reference keeps in KLT_Feature (klt.py:255-263); the three (window+2)^2 templates live in a
 * device array next to these records */
typedef struct { float aff_x, aff_y, Axx, Ayx, Axy, Ayy; int32_t valid, pad /* Newton iterations of the feature's last check */; } klt_affine_rec;
int klt_set_affine_params(klt_ctx *ctx, const klt_affine_params *p);
int klt_affine_alloc(klt_ctx *ctx, int state, int n);          /* n feature slots, no templates yet */
int klt_affine_download(klt_ctx *ctx, int state, klt_affine_rec *dst, int n);
/* device-side snapshot: the records (and, with_templates != 0, the templates) of the first n features of state `src` into `dst`
 * (allocated if needed), on the context's stream.  The templates of a feature never change while its record is valid. */
int klt_affine_copy_async(klt_ctx *ctx, int dst, int src, int n, int with_templates);
int klt_affine_free(klt_ctx *ctx, int state);                  /* releases records + templates; the id can be allocated again */
/* klt_track_async followed by the consistency check of the features it tracked; fb_in != fb_out.  `state` travels
 * with the feature list (same index = same feature). */
int klt_track_affine_async(klt_ctx *ctx, int slot1, int slot2, int fb_in, int fb_out, int n, int state);
int klt_track_affine(klt_ctx *ctx, int slot1, int slot2, klt_feat *inout, int n, int state, int *n_tracked);

typedef struct {
    uint64_t features;                       /* live features entering the kernel */
    uint64_t level_visits[KLT_MAX_LEVELS];   /* _trackFeature calls per pyramid level */
    uint64_t iterations[KLT_MAX_LEVELS];     /* Newton iterations per pyramid level */
} klt_track_stats;
/* reset zeroes the counters and starts collecting (a small reduction kernel after every tracker launch);
 * read returns the totals since the reset and stops collecting.  klt_feat.aux of a tracked record holds
 * 4 bits per level: 0 = level not visited, v = v-1 Newton iterations (saturating at 14). */
int klt_track_stats_reset(klt_ctx *ctx);
int klt_track_stats_read(klt_ctx *ctx, klt_track_stats *out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (BASELINE cfg-4) --------------------- */
/* The reference has no counterpart (single process, single thread; its only concurrency is the GUI's multiprocessing
 * queue, examplegui.py:22-29).  The path shards by frame pair, so ranks never exchange pixels: the only collective is
 * the gather of 16-byte feature records at the end of a shard.  librccl is opened on first use (dlopen); a process that
 * never calls these entry points never loads it.  Collectives run on a side stream of the context, event-ordered behind
 * everything enqueued on the context's stream when they are issued; the context's stream itself never waits for RCCL
 * unless klt_comm_fence_async is called. */
#define KLT_COMM_ID_BYTES 128
/* rank 0: a fresh RCCL unique id (ncclGetUniqueId); the caller hands the 128 bytes to the other ranks (file, socket, env) */
int klt_comm_unique_id(void *out128);
/* every rank, same id: joins the communicator of `nranks` processes (ncclCommInitRank on the context's device) */
int klt_comm_init_rank(klt_ctx *ctx, int nranks, int rank, const void *unique_id);
int klt_comm_destroy(klt_ctx *ctx);
int klt_comm_info(klt_ctx *ctx, int *nranks, int *rank);       /* 1 / 0 when the context has no communicator */
/* all-gather / gather of the first n records of feature buffer fb_src into fb_dst (nranks * n records in rank order;
 * allocated here if needed; for the gather only `root` needs / gets fb_dst, other ranks may pass -1).  n may cover a
 * whole device-side [pairs x features] table (klt_featbuf_view). */
int klt_allgather_featbuf_async(klt_ctx *ctx, int fb_src, int fb_dst, int n);
int klt_gather_featbuf_async(klt_ctx *ctx, int fb_src, int fb_dst, int n, int root);
/* gather with a count per rank (shards of unequal size: 7 or 257 pairs over 8 GPUs): rank r contributes the first counts[r]
 * records of its fb_src, the root's fb_dst receives sum(counts) records back to back in rank order.  Every rank passes the same
 * table of nranks counts; a rank with count 0 takes no part in the transfer (its fb_src may be -1). */
int klt_gatherv_featbuf_async(klt_ctx *ctx, int fb_src, int fb_dst, const int *counts, int root);
/* The feature list as the baton of ONE temporal sequence cut into blocks of frames, one block per GPU (the tracker and the
 * replacement pass are a serial chain, trackFeatures.py:250-346 / selectGoodFeatures.py:45-135; everything that depends on the pixels
 * only is prepared by the block's owner meanwhile): n records of fb_send go to rank `to` and / or n records from rank `from` arrive in
 * fb_recv (-1: no such side; to == from == own rank: a device copy), on the side stream behind everything enqueued on the context's
 * stream so far; the context's stream then waits for the arrival.  fb_send must stay untouched until klt_comm_fence_featbuf_async. */
int klt_sendrecv_featbuf_async(klt_ctx *ctx, int fb_send, int to, int fb_recv, int from, int n);
int klt_comm_fence_async(klt_ctx *ctx);    /* the context's stream waits (on the device) for the collectives issued so far */
/* ... only for the last collective that read or wrote feature buffer fb (call it before overwriting a table whose
 * gather may still be in flight; collectives on other tables keep overlapping) */
int klt_comm_fence_featbuf_async(klt_ctx *ctx, int fb);
int klt_comm_wait(klt_ctx *ctx);           /* the host waits for them -- at most the communicator's timeout, then KLT_ERR_TIMEOUT */
/* Host-side waits on the communicator (klt_comm_wait, klt_sync, klt_comm_allreduce_max, and the waits before device memory that a
 * collective may touch is freed) give up after `ms` milliseconds with KLT_ERR_TIMEOUT instead of hanging when a peer has died;
 * default 300 000, or KLT_COMM_TIMEOUT_MS in the environment; <= 0 waits for ever.  After a timeout the communicator is unusable:
 * the rank should report and exit non-zero (never restart in place a process that has touched the GPU). */
int klt_comm_set_timeout(klt_ctx *ctx, double ms);
/* element-wise maximum over all ranks of n <= 16 doubles (host in, host out; synchronous -- also the barrier the
 * benchmark brackets its timed region with) */
int klt_comm_allreduce_max(klt_ctx *ctx, double *inout, int n);

/* ---- test / inspection hooks --------------------------------------------------------------- */
/* pyramid: 0 = image, 1 = gradx, 2 = grady; dst holds level_ncols*level_nrows floats.  (On the device the three planes of a level are
 * stored as pixel records -- image, gradx, grady of a pixel side by side, DESIGN.md section 5 --; this call and klt_download_select_f32 hand
 * out separate planes.) */
int klt_level_dims(klt_ctx *ctx, int slot, int level, int *ncols, int *nrows);
int klt_download_f32(klt_ctx *ctx, int slot, int pyramid, int level, float *dst);
/* selection intermediates of the last klt_select*: 0 = smoothed image, 1 = gradx, 2 = grady (full frame),
 * 3 = eigenvalue map [ny][nx] (scan order, goodFeaturesUtils.pyx:53-54; after a KLT_REPLACING_SOME selection the pixels inside
 * the exclusion squares of the live features read 0, as do the candidates a selection mask excludes: they can never be placed and are not scored; a selection that used the
 * scores of klt_select_prepare_async writes no map, and 3 is refused after it).  dims via klt_select_dims. */
int klt_select_dims(klt_ctx *ctx, int what, int *ncols, int *nrows);
int klt_download_select_f32(klt_ctx *ctx, int what, float *dst);
/* the NEXT klt_select* takes `count` = nx*ny eigenvalues from `val` (scan order, as what = 3 above returns them) instead
 * of computing them: lets the tests drive _enforceMinimumDistance (selectGoodFeatures.py:45-135) with equal scores and
 * long dependency chains that real frames rarely contain.  The override is consumed by one selection. */
int klt_set_score_override(klt_ctx *ctx, const float *val, int count);
/* first `n` sorted candidates of the last klt_select* as (val, x, y), selectGoodFeatures.py:234-236 */
int klt_download_sorted_candidates(klt_ctx *ctx, float *val, int32_t *x, int32_t *y, int n, int *n_valid);
/* Diagnostic, read-only: the keys of the score set that klt_select_prepare_async prepared for the slot's CURRENT contents under the current
 * selection parameters -- nx * ny 64-bit keys in scan order (y outer, x inner: key k belongs to the candidate at x = borderx + (k % nx) *
 * step, y = bordery + (k / nx) * step), each the f32 bits of val << 32 | x << 16 | y as klt_download_sorted_candidates describes them,
 * or 0 where (double)val < max(min_eigenvalue, 1).  Waits (on the host) for the set's own event; the set is NOT consumed and nothing is
 * enqueued.  KLT_ERR_STATE when no set matches (none prepared, already used by a selection, the slot rebuilt or the parameters changed
 * since); KLT_ERR_ARG when capacity (in keys) < nx * ny -- *nx and *ny (either may be NULL) are set then as well, so a caller can size
 * the buffer and repeat. */
int klt_download_prepared_keys(klt_ctx *ctx, int slot, uint64_t *dst, size_t capacity, int *nx, int *ny);
/* Diagnostic, read-only: which kernels built the summed-area tables of the most recent klt_select_prepare_async or klt_select* that built
 * any (a selection that used prepared scores builds none and leaves the preparation's codes), recorded where the launch decisions are
 * made, the fallback after the fused kernel declines a geometry included.  KLT_ERR_STATE before the first.  Either pointer may be NULL.
 * The choice depends on KLT_OPT_SAT_VARIANT, ncols % 4, the window, nSkippedPixels and KLT_FUSED_COLS_EIGEN in the environment; every
 * path gives the same tables and keys bit for bit -- the tests use this to know that the kernel they were written for is the one that ran. */
#define KLT_SCORE_BARRIER 0         /* *rows, *cols: sat_rows_kernel / sat_cols_kernel (KLT_OPT_SAT_VARIANT 0, or ncols % 4 != 0) */
#define KLT_SCORE_PIPELINE 1        /* *rows, *cols: sat_rows_pipe / sat_cols_pipe */
#define KLT_SCORE_FUSED_KEYS 2      /* *cols only: cols_eigen_pipe, the column pass and the eigenvalue keys in one launch (klt_select_prepare_async) */
int klt_select_score_path(klt_ctx *ctx, int *rows, int *cols);
/* Diagnostic, read-only: how the last COMPLETED selection (klt_select, klt_select_async, klt_select_begin_async + klt_select_finish) got
 * from the eigenvalue keys to the list, recorded where the decisions are taken; nothing is enqueued.  KLT_ERR_STATE before the first, and
 * while a selection is pending.  Every path gives the same list -- the tests use this to know that the code they were written for ran. */
typedef struct klt_select_pick {
    int32_t walk;            /* 0: sorted serial walk; 1: parallel minimum-distance passes */
    int32_t order;           /* 0: the greedy walk alone; 1: accepted candidates ranked by counting; 2: accepted keys sorted, then walked */
    int32_t cut;             /* 1: the top-K prefilter was planned (more than 262144 candidates and a target below half of them) */
    int32_t attempts;        /* 1, or 2: the cut's candidates ran out and the selection was repeated with every candidate */
    int32_t passes;          /* parallel: minimum-distance passes launched, both attempts; serial: 0 */
    int32_t looks;           /* parallel: times the host looked at the outcome; serial: 0 */
    int32_t instantiation;   /* parallel: 9 (the radius compiled in) or 0 (any radius); serial: 0 */
    int32_t pass_lds;        /* parallel: dynamic LDS bytes of a pass; serial: 0 */
    int32_t grid;            /* cell grid of the greedy walk, where one ran: 0 in LDS, 1 in global memory */
    int32_t sparse;          /* parallel: 1 when the later passes took several tiles per workgroup (a replacement behind the cut) */
} klt_select_pick;
int klt_select_pick_path(klt_ctx *ctx, klt_select_pick *out);

/* ---- standalone convolutions (host buffers in / out, synchronous) ---------------------------- */
/* _convolveSeparate(imgin, horiz_kernel, vert_kernel), convolve.py:208-219 (SciPy branch: scipy.ndimage.convolve1d along axis 1, then
 * along axis 0; FP64 accumulation in correlate1d's operation order, f32 after each pass, `reflect` borders): the reference's one general
 * separable convolution -- ANY two tap lists of 1 .. 71 taps, odd or even (an even count shifts the window as convolve1d does), symmetric,
 * antisymmetric or neither.  f32 image in, f32 image out. */
int klt_convolve_separate_f32(klt_ctx *ctx, const float *src, int ncols, int nrows, const double *horiz, int nh, const double *vert, int nv,
                              float *dst);
/* KLTComputeSmoothedImage, convolve.py:254-264: _convolveSeparate(img, gauss, gauss) */
int klt_smooth_f32(klt_ctx *ctx, const float *src, int ncols, int nrows, const double *gauss, int ng, float *dst);
/* KLTComputeGradients, convolve.py:226-248: gradx = (deriv, gauss), grady = (gauss, deriv) */
int klt_gradients_f32(klt_ctx *ctx, const float *src, int ncols, int nrows, const double *gauss, int ng,
                      const double *deriv, int nd, float *gradx, float *grady);

/* KLTPyramid.Compute, pyramid.py:37-77: level 0 = src unchanged; level i = level i-1 smoothed with `gauss` (the taps of sigma =
 * subsampling * sigma_fact, convolve.py:27-93) and sampled at (ss y + ss/2, ss x + ss/2), dimensions int(n / ss).  dst receives
 * levels 1 .. nlevels-1 back to back (nothing for nlevels = 1); all levels stay on the device until the one download. */
int klt_pyramid_f32(klt_ctx *ctx, const float *src, int ncols, int nrows, int nlevels, int subsampling, const double *gauss, int ng,
                    float *dst);

/* ---- the reference's literal native boundary (host arrays in / out, synchronous) --------------- */
/* The only FFI the reference really has is its Cython `def` layer (setup.py:8-9).  These three are its entry points on the hot
 * path, bound by pyfeaturetrack_amd/compat/goodFeaturesUtils.py and trackFeaturesUtils.py under the reference's module and
 * function names.  Every call uploads the planes it is given: a boundary for drop-in use and for parity checks at the reference's
 * own granularity, not the fast path (that is klt_select* / klt_track*). */
/* ScanImageForGoodFeatures, goodFeaturesUtils.pyx:35-73: summed-area tables of gradx^2, gradx grady, grady^2 (f32 sequential scans,
 * :49-51) and the minimum eigenvalue of every candidate window (:17-31), candidates at x = borderx, borderx + step, ... < ncols - borderx
 * (the same in y), step = nSkippedPixels + 1.  val receives nx * ny eigenvalues in scan order (y outer, x inner: the order of the
 * reference's three lists); *nx, *ny the grid.  Arguments are the C ints Cython truncates the Python floats to (30.0 -> 30, 3.5 -> 3). */
int klt_scan_good_features_f32(klt_ctx *ctx, const float *gradx, const float *grady, int ncols, int nrows, int borderx, int bordery,
                               int window_hw, int window_hh, int nSkippedPixels, float *val, int val_cap, int *nx, int *ny);
/* extractImagePatchSlow, trackFeaturesUtils.pyx:14-51: width x height bilinear samples around (x, y), weights in FP64.
 * Square patches only (the reference swaps the roles of rows and columns, :38-49); a footprint that leaves the image is KLT_ERR_ARG
 * (the reference asserts, :35). */
int klt_extract_patch_f32(klt_ctx *ctx, const float *img, int ncols, int nrows, float x, float y, int width, int height, float *patch);
/* trackFeatureIterateCKLT, trackFeaturesUtils.pyx:393-459: the Newton loop of one feature at one pyramid level on template patches
 * the caller extracted; returns the position, the status (KLT_TRACKED / KLT_OOB / KLT_SMALL_DET) and the iteration count.  The tests
 * after the loop and the status priority are _trackFeature's (trackFeatures.py:67-136), i.e. the caller's.  Square windows only
 * (the reference's jacobian is strided by shape[0], :128). */
int klt_track_iterate_f32(klt_ctx *ctx, float x2, float y2, const float *gradx_patch, const float *grady_patch, const float *img_patch,
                          int width, int height, const float *img2, const float *gradx2, const float *grady2, int ncols, int nrows,
                          float step_factor, float min_determinant, float min_displacement, int max_iterations,
                          float *x2_out, float *y2_out, int *status, int *iterations);

/* ---- per-kernel timing (HIP events on the context's stream) -------------------------------- */
typedef struct { char name[32]; uint32_t launches; float total_ms; double bytes; } klt_kernel_time;
int klt_timing_enable(klt_ctx *ctx, int on);                /* resets the accumulated figures.  1: an event pair around every launch;
                                                             * 2: the same, but the kernels that are one launch per call (smooth_grad_l0, pyramid_reduce, gradients, track,
                                                             * affine_check, sat_rows, sat_cols, eigen_keys) are timed by their dispatch's own begin / end timestamps
                                                             * (hipExtLaunchKernelGGL events) -- the kernel duration a profiler reports, without the boundary between
                                                             * two dependent launches that an event pair also holds */
int klt_timing_read(klt_ctx *ctx, klt_kernel_time *out, int max_entries);   /* returns the entry count.  Mode 2: a launch of a stamped family that took
                                                                              * a path without dispatch timestamps (a fallback kernel) is not measured; such
                                                                              * launches are counted in an extra entry "<family>!unstamped" (no time) */

#ifdef __cplusplus
}
#endif
#endif /* KLT_GPU_H */
