// klt_context.h -- what the files of the C ABI (api_*.hip) share: the context object behind `klt_ctx` with its slots, feature buffers and
// selection state, the error / timing helpers, and the declarations of the helpers one file defines and another uses.  Host-side C++
// only; the kernels and their launchers are declared in klt_internal.h.  Everything lives in namespace kltapi except klt_ctx itself
// (the opaque type of include/klt_gpu.h).
//
//   api_context.hip   lifetime, parameters, options, slots' state, events and buffers every other file leans on, timing
//   api_frames.hip    frames in (uploads, pinned / device memory, adoption), pyramid build, stand-alone convolutions, plane read-back
//   api_featbuf.hip   feature buffers: copies either way, views, host-mapped buffers
//   api_select.hip    selection: score preparation, the begin / finish protocol, the given-list walk, its inspection hooks
//   api_track.hip     tracker launches (single pair, batched), constant-velocity prediction, iteration counters
//   api_quality.hip   per-feature track quality (single pair, batched)
//   api_consensus.hip the consensus checks -- motion model, epipolar, homography -- (single pair, batched), their model records in pixels
//   api_crowd.hip     crowding check (single list, batched)
//   api_describe.hip  binary descriptors of a slot's 8-bit frame and their Hamming matcher
//   api_reacquire.hip track identities over a sequence: the bank of lost tracks and their re-acquisition
//   api_affine.hip    affine consistency check and its per-feature state
//   api_comm.hip      the multi-GPU entry points (RCCL itself: comm.hip)
//   api_compat.hip    the reference's literal native boundary (one call = one wavefront), the HIP-graph experiment
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "klt_internal.h"
#include "ingest_rule.h"

struct klt_ctx;

namespace kltapi {


enum Family { F_SMOOTH_GRAD, F_PYR_REDUCE, F_GRAD, F_SMOOTH_H, F_SMOOTH_V, F_PYR_H, F_PYR_V, F_GRAD_H, F_GRAD_V, F_TRACK,
              F_SAT_ROWS, F_SAT_COLS, F_EIGEN, F_SORT, F_NMS, F_SEED, F_AFFINE, F_CROWD_PREPARE, F_CROWD, F_EQ_LUT, F_EQ_APPLY, F_REMAP, F_DESCRIBE, F_MATCH, F_MATCH_RESOLVE,
              F_REACQ_CLASSIFY, F_REACQ_BANK, F_REACQ_FRESH, F_REACQ_ASSIGN, F_COUNT };
inline const char *const kFamilyName[F_COUNT] = {"smooth_grad_l0", "pyramid_reduce", "gradients", "smooth_h", "smooth_v", "pyramid_h",
                                          "pyramid_v", "gradient_h", "gradient_v", "track", "sat_rows", "sat_cols",
                                          "eigen_keys", "sort", "nms", "seed_map", "affine_check", "crowd_prepare", "crowd_check", "equalize_lut", "equalize_apply", "remap", "describe", "match", "match_resolve",
                                          "reacquire_classify", "reacquire_bank", "reacquire_fresh", "reacquire_assign"};

struct Level { int nc = 0, nr = 0; float *img = nullptr, *gx = nullptr, *gy = nullptr; };

// One of a slot's two alternating raw buffers with everything that orders work on it (Slot::raw, Slot::raw_alt: an asynchronous upload
// exchanges the two whole)
struct RawBuffer {
    uint8_t *u8 = nullptr;
    size_t cap = 0;                   // bytes
    hipEvent_t ev_consumed = nullptr; // last kernel on `stream` that read the raw frame in it
    uint64_t consumed_serial = 0;     // when the ring handed that event out (event_live)
    bool consumed_valid = false;
    // last asynchronous copy INTO the buffer (consecutive uploads go round-robin over the copy streams: the next copy into the same
    // buffer may be issued on another stream and must wait for this one)
    hipEvent_t ev_wr = nullptr;
    uint64_t wr_serial = 0;
    int wr_lane = -1;
};

// The points of the ingest chain in their order: the frame as it came, its remapped copy (klt_set_remap), its equalised copy
// (klt_set_equalize_params).  A stage reads the output of the last stage in front of it that is switched on (ingest_output)
enum IngestStage { INGEST_FRAME, INGEST_REMAP, INGEST_EQUALIZE };

struct Slot {
    int nc = 0, nr = 0;
    int raw_kind = 0;                 // 0 none, 1 u8, 2 f32
    float *f32 = nullptr;
    size_t f32_cap = 0;               // pixels
    float *planes = nullptr;          // 3 pyramids, level-concatenated
    size_t planes_cap = 0;            // floats
    Level lv[KLT_MAX_LEVELS];
    int nlev = 0, ss = 0;
    bool pyr_valid = false;
    // KLT_OPT_L0_LAZY_GRAD: the compact level-0 image a lean build writes instead of the level-0 records (nc x nr floats, allocated on
    // the slot's first lean build).  A built slot has valid level-0 records (rec0_valid), a valid compact image (l0img_valid), or --
    // once ensure_level0_records has made the records of a lean build -- both.
    float *l0img = nullptr;
    size_t l0img_cap = 0;             // floats
    bool rec0_valid = false, l0img_valid = false;
    // since the slot's last build: a tracker launch that has a lazy form read it / something asked for its level-0 records
    bool lazy_read = false, rec0_asked = false;
    int built_nc = 0, built_nr = 0;   // frame size and taps / pyramid shape (klt_ctx::cfg_gen) of that build: a change of either resets
    uint64_t built_cfg = 0;           // the slot to a full build
    uint64_t gen = 0;                // which build filled the pyramids (unique per build; travels with klt_swap_slots)
    hipEvent_t ev_upload = nullptr;   // asynchronous ingest: frame copy finished (the build waits for it)
    uint64_t upload_serial = 0;       // when the ring handed that event out (event_live)
    hipEvent_t ev_built = nullptr;    // KLT_OPT_BUILD_STREAM: end of the build that filled this slot's pyramids (recorded on the build stream)
    uint64_t built_serial = 0;
    bool built_pending = false;       // the main stream has not waited for ev_built yet
    bool built_on_bstream = false;    // which stream the last build of this slot ran on
    hipEvent_t ev_read = nullptr;     // last tracker launch on the main stream that reads this slot's pyramids (a build on the build
    uint64_t read_serial = 0;         // stream waits for it; selections synchronise before they return and need no mark)
    bool read_valid = false;
    bool upload_pending = false;
    // asynchronous ingest alternates between two raw buffers so that a copy never has to wait (on the device) for
    // kernels still reading the previous frame: making the copy stream wait on a compute-stream event blocks the
    // HOST for the duration of the queued work on this runtime (measured 150-800 us per step)
    RawBuffer raw, raw_alt;           // the buffer that holds (or is receiving) the slot's frame, and the other one
    const uint8_t *u8_ext = nullptr;  // klt_slot_adopt_u8: the frame IS this caller-owned device buffer (read in place, never written or freed here)
    bool f32_in_raw = false;          // klt_upload_f32_async: the f32 frame lives in the alternating raw buffers (`raw.u8`, 4 bytes per pixel), not in `f32`
    // klt_set_equalize_params, mode 1: the equalised copy of the 8-bit frame (nc x nr bytes, rounded up to 256) with the per-tile LUTs
    // it was made from behind it, allocated when first needed.  eq_valid: it was made from the frame the slot holds now -- this upload or
    // adoption -- under the parameters the context holds now (a new frame, klt_slot_free or new parameters clear it)
    uint8_t *eq = nullptr;
    size_t eq_cap = 0;                // bytes
    bool eq_valid = false;
    // klt_set_remap: the remapped copy of the 8-bit frame (nc x nr bytes), allocated when first needed.  rm_valid: it was made from the
    // frame the slot holds now under the map the context holds now.  What clears the two flags: void_copies_from, nothing else
    uint8_t *rm = nullptr;
    size_t rm_cap = 0;                // bytes
    bool rm_valid = false;
    // a frame arrives (every upload, adoption) / the slot holds no frame any more (api_frames.hip)
    void take_frame(int ncols, int nrows, int kind, bool in_raw);
    void drop_frame();
};

inline const float *rawf(const Slot *s) { return s->f32_in_raw ? reinterpret_cast<const float *>(s->raw.u8) : s->f32; }

struct FeatBuf { klt_feat *d = nullptr; int cap = 0; bool view = false; hipEvent_t comm_done = nullptr; /* last collective that touched it */ };

struct AffState { klt_affine_rec *rec = nullptr; float *tpl = nullptr; int n = 0, tn = 0; };

// The feature buffers behind the synchronous entry points (klt_track, klt_select, klt_track_quality, ...): staging for the caller's
// arrays -- the list in, the list out, the backward records, the guesses, and the private record buffer of klt_track_quality (quality
// records) and klt_motion_check (the model record).  One set serves them all, the last one two of them: every synchronous entry point
// has downloaded what it wants before it returns, so no two of them are ever in flight on these buffers.
// ... and the two descriptor buffers of the track identities (P and Q, exchanged every step: api_reacquire.hip)
constexpr int kFbReacqDesc[2] = {29991, 29990};
constexpr int kFbSyncIn = 65534, kFbSyncOut = 65535, kFbSyncBack = 65532, kFbSyncGuess = 65531, kFbSyncOwn = 65530;

// The descriptor table of a batched launch that stays on the device and is sent again only when it differs (send_if_changed)
template <class Desc>
struct SentTable {
    std::vector<Desc> host;           // what `dev` holds
    Desc *dev = nullptr;
    size_t cap = 0;
};

// What a consensus check over feature lists keeps in the context (api_consensus.hip): its parameters as the caller set them (the fields
// klt_model_params, klt_epipolar_params and klt_homography_params share; min_area is the first one's alone), which form its last launch
// took (klt_*_check_path), and its candidates and scores in one scratch allocation, a slice per pair, behind the table of a batched launch
struct ConsensusParams { int32_t mode, ncols, nrows, hypotheses; uint32_t seed; int32_t min_inliers; float max_error, min_area; };
struct ConsensusState {
    ConsensusParams p;
    int path = 0;
    unsigned char *scratch = nullptr;
    size_t scratch_cap = 0;
    SentTable<ModelPair> table;
};

struct Timed { int fam; hipEvent_t a, b; double bytes; };

extern std::string g_create_error;      // klt_create has no context to report into (api_context.hip)


// one set of prepared selection scores (klt_select_prepare_async)
struct ScoreCache {
    unsigned long long *keys = nullptr;
    size_t cap = 0;
    uint64_t gen = 0, stamp = 0;      // generation of the slot contents the keys were scored on (0 = empty); age
    int nc = 0, nr = 0, bx = 0, by = 0, hw = 0, hh = 0, step = 0, nx = 0, ny = 0;
    double min_eig = 0;
    hipEvent_t ev = nullptr;
    uint64_t ev_serial = 0;
};

// The parallel minimum-distance selection in two halves: everything up to the point where the host has to look at the outcome
// (klt_select_begin_async) and the rest (klt_select_finish: wait, look, and -- rarely -- more passes or the repeat with every
// candidate).  Between the two the caller may enqueue other work (the next frame's upload, build and score preparation).
struct SelectJob {
    static constexpr int kMaxRounds = 512;
    MisArgs ma;
    NmsArgs pa;
    SelectArgs sa;
    klt_feat *fl = nullptr;
    ScoreCache *pre = nullptr;
    unsigned *zero_from = nullptr, *hist_d = nullptr, *ticket_d = nullptr, *info_d = nullptr, *rank_d = nullptr, *acc_count_d = nullptr;
    int *nfill_d = nullptr;
    size_t zero_n = 0;
    long long bound = 0, np2 = 0, ncand = 0, target = 0;
    int n = 0, mode = 0, rounds_per_look = 0, attempt = 0, round = 0, look = 0;
    int passes = 0;                           // passes launched, both attempts (klt_select_pick_path)
    bool by_rank = false, prefilter = false, filtered = false;
    bool quota = false;                       // a grid is set (klt_set_select_grid): qa, and the frame the cells lie on
    QuotaArgs qa{};
    int ncols = 0, nrows = 0;
    int cut_scale = 1;                        // the factor a grid widens the prefilter's cuts by (KLT_GRID_CUT_SCALE)
};


}  // namespace kltapi

using namespace kltapi;      // (this header is for the api_*.hip files only)

struct klt_ctx {
    int device = -1;
    klt_equalize_params eqp{0, 8, 8, 768};    // CLAHE ingest stage (klt_set_equalize_params): off; 8 x 8 tiles, clip limit 3.0
    int eq_path = 0;                          // klt_equalize_path: the last build enqueued equalisation launches
    // remap ingest stage (klt_set_remap): the context's one map, two planes of nc * nr int32 in one allocation (x first; the y plane
    // begins on a 256-byte boundary), uploaded synchronously by the set call and freed with the context.  d == nullptr: the stage is off
    struct RemapTable { int32_t *d = nullptr; size_t plane = 0; /* int32 from x to y */ int nc = 0, nr = 0; } rmp;
    int rm_path = 0;                          // klt_remap_path: the last build enqueued a remap launch
    hipStream_t stream = nullptr;     // uploads, pyramid build, selection, tracker
    hipStream_t cstream = nullptr;    // asynchronous frame ingest from pinned host memory (created on first use)
    // ... and more copy streams: consecutive uploads go round-robin over all of them, i.e. over several DMA engines (2 MB frames: 44 GB/s
    // on one stream, 55 GB/s on two -- profiles/r04_h2d_probe.json), and a stream's next copy is not queued right behind the event of its last one
    static constexpr int kMaxCopyStreams = 8;
    hipStream_t cextra[kMaxCopyStreams - 1] = {nullptr};
    int ncopy = 2;                    // copy streams in use (KLT_COPY_STREAMS)
    unsigned upload_count = 0;
    hipStream_t bstream = nullptr;    // KLT_OPT_BUILD_STREAM: pyramid builds run here, overlapping the tracker / selection of earlier frames
    hipStream_t work = nullptr;       // stream the pyramid-build helpers enqueue on: `stream`, or `bstream` inside a build
    bool build_stream_on = false;
    KltComm *comm = nullptr;          // RCCL communicator + side stream (klt_comm_init_rank), comm.hip
    std::vector<void *> pinned;       // klt_host_alloc allocations
    std::vector<void *> dev_allocs;   // klt_device_alloc allocations
    std::vector<size_t> dev_alloc_bytes;
    // Ordering events come from one ring and are never re-recorded while a waiter may still be queued on them
    // (re-recording a pending event makes hipEventRecord block the host until the device has caught up -- measured:
    // 400-800 us per step).  256 events ~ 25 steps of history.
    std::vector<hipEvent_t> ring;
    size_t ring_next = 0;
    uint64_t ring_serial = 0;         // events handed out so far
    std::string err;
    klt_params p{};
    bool have_params = false;
    Taps gauss[3], deriv[3];
    bool have_taps[3] = {false, false, false};
    std::vector<Slot> slots;
    std::vector<FeatBuf> fbs;
    float *tmpA = nullptr, *tmpB = nullptr;
    size_t tmp_cap = 0;
    float *h1 = nullptr;                      // H1 planes of the fused first reduction (one per frame of a batch)
    size_t h1_cap = 0;
    float *cimg = nullptr;                    // compact image planes of a pyramid build's levels (what the reductions read and write)
    size_t cimg_cap = 0;
    bool fuse_hreduce = true;                 // KLT_OPT_FUSED_HREDUCE
    int l0_stream = 2;                        // KLT_OPT_L0_STREAM: 0 tiled, 1 streaming, 2 (default) streaming with wide strips where they apply
    int l0_path = -1;                         // klt_level0_path: KLT_L0_* of the last geometry group of the last build (-1: no build yet)
    bool l0_merged_grad = false;              // ... and whether that group's gradients of levels >= 1 went out as one launch
    int l0_lazy_grad = 1;                     // KLT_OPT_L0_LAZY_GRAD: 0 never lean, 1 adaptive, 2 lean wherever a streaming kernel is launched
    bool l0_lean = false;                     // klt_level0_lean: that group went out lean
    int l0_lean_form_opt = KLT_L0_LEAN_FORM_DEFAULT;   // KLT_OPT_L0_LEAN_FORM: 1 the wave form where it applies, 0 the banded form
    int l0_lean_form = 0;                     // klt_level0_lean_form: 0 not lean, 1 banded, 2 wave (that group's launch)
    uint64_t cfg_gen = 1;                     // counts the changes of the taps and of the pyramid's shape (Slot::built_cfg)
    bool track_xcd_order = true;              // KLT_OPT_TRACK_XCD_ORDER
    int track_lazy_form = KLT_TRACK_LAZY_FORM_DEFAULT;   // KLT_OPT_TRACK_LAZY_FORM: 1 the fused level-0 entry phase of the lazy tracker, 0 two calls
    uint64_t waited_built_serial = ~0ull;     // the build event the main stream waited for last (wait_built)
    // selection scratch
    float *sel_img = nullptr, *sel_rec = nullptr, *sat = nullptr, *valmap = nullptr;   // compact image, pixel records (KLT_PIX_STRIDE)
    size_t sel_cap = 0;               // pixels
    unsigned long long *keys = nullptr;
    size_t keys_cap = 0;
    uint8_t *seedmap = nullptr;
    size_t seed_cap = 0, seed_n = 0;          // pixels the stamps in the map are valid for
    uint8_t seed_stamp = 0;                   // stamp of the latest selection that used the map (1..255)
    // selection mask (klt_set_select_mask*): what the selections read -- the context's own plane (a host mask's copy) or the caller's
    // device memory, [mask_nr][mask_nc] bytes without padding between rows; null = no mask
    const uint8_t *mask = nullptr;
    int mask_nc = 0, mask_nr = 0;
    uint8_t *mask_own = nullptr;
    size_t mask_own_cap = 0;
    // per-cell quota of the selector (klt_set_select_grid): cell_width == 0 = no grid.  quota_buf, for a frame of `cells` cells:
    // [3 * cells] 64-bit words of the filter's rounds | [cells] live counts | the number of keys the filter kept
    klt_select_grid sel_grid{0, 0, 0};
    int grid_path = 0;                        // klt_select_grid_path
    unsigned long long *quota_buf = nullptr;
    size_t quota_buf_cap = 0;
    uint32_t *grid = nullptr;
    size_t grid_cap = 0;
    int *nms_slots = nullptr;
    size_t nms_slots_cap = 0;
    unsigned long long *keys2 = nullptr;      // compacted top-K keys
    size_t keys2_cap = 0;
    unsigned *topk_hist = nullptr;            // 8192 bins + 4 words of info
    klt_feat *fl_snapshot = nullptr;
    size_t fl_snapshot_cap = 0;
    bool track_tree_sums = false;     // KLT_OPT_TRACK_TREE_SUMS
    bool use_topk = true;
    bool use_mis = true;                      // parallel minimum-distance passes instead of the sorted serial walk
    int mis_rounds_hint = 6;
    int sat_variant = 1;                      // 1: step-synchronous wavefront pipelines (sat_pipeline.hip), 0: barrier-coupled SAT kernels
    int score_rows_path = -1, score_cols_path = -1;   // klt_select_score_path: KLT_SCORE_* of the tables' row / column pass last enqueued (-1: none yet)
    klt_select_pick pick{-1, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // klt_select_pick_path: how the last completed selection picked (walk -1: none yet)
    unsigned *readback = nullptr;             // pinned scratch for small results
    float *score_override = nullptr;          // test hook (klt_set_score_override)
    size_t score_override_cap = 0;
    int score_override_n = 0;
    uint32_t *mis_st = nullptr, *mis_list = nullptr;
    unsigned long long *mis_tile_keys = nullptr;
    size_t mis_tile_keys_cap = 0;
    unsigned *mis_cnt = nullptr;              // [tiles] + kMisRounds remaining counters + accepted counter
    size_t mis_st_cap = 0, mis_list_cap = 0, mis_cnt_cap = 0;
    // klt_select_prepare_async: the list-independent half of a selection (summed-area tables, eigenvalue keys) of a slot's level 0, computed
    // ahead of time (on the build stream when that is on).  Two sets by default: the next frame's keys are written while this frame's are read;
    // a rank that prepares a whole block of frames while it waits for the feature list of the previous block keeps one per frame.
    std::vector<ScoreCache> pre = std::vector<ScoreCache>(2);      // KLT_OPT_SCORE_SETS
    std::unique_ptr<SelectJob> sel_job;       // a selection between klt_select_begin_async and klt_select_finish
    hipEvent_t ev_download = nullptr;         // behind the latest klt_featbuf_download_async (an event of the ring)
    uint64_t download_serial = 0;
    bool download_pending = false;
    hipEvent_t ev_sel = nullptr;              // behind the last launch of the pending selection's latest batch: what klt_select_finish waits for
    float *sat_pre = nullptr;
    size_t sat_pre_cap = 0;
    uint64_t gen_counter = 0, pre_stamp = 0;
    int last_build_on_bstream = -1;           // -1: no build yet
    hipEvent_t ev_bbuild = nullptr;           // end of the latest build on the build stream (shares the H1 scratch with main-stream builds)
    uint64_t bbuild_serial = 0;
    const unsigned long long *sorted_keys = nullptr;   // what the last selection walked (test hook)
    int sorted_count = 0;
    // batched tracker launches: the descriptor tables (and XCD-aware feature orders) of the last few distinct batches stay on the device --
    // a shard that goes through in sub-shards, step after step, uploads each table once
    struct BatchTable {
        std::vector<TrackPairDesc> host;          // what `dev` holds
        uint64_t hash = 0;
        TrackPairDesc *dev = nullptr;
        size_t cap = 0;
        uint64_t used = 0;
    };
    // the XCD-aware feature orders depend on the INPUT lists only: one set of permutations per distinct (inputs, length), whatever
    // the frames and the output buffers of the launch
    struct BatchOrder {
        std::vector<const klt_feat *> in;
        uint32_t *order = nullptr;
        size_t cap = 0;
        int n = -1, age = 0;
        uint64_t used = 0;
    };
    std::vector<BatchTable> batch_tables;         // at most kBatchTables, least recently used one replaced
    std::vector<BatchOrder> batch_orders;         // at most kBatchOrders
    BatchOrder shared_order;                      // single-pair launches on lists seen for the first time
    std::vector<const klt_feat *> seen_once;      // input lists of single-pair launches seen once so far (set_track_order)
    uint64_t batch_clock = 0;
    static constexpr size_t kBatchTables = 256, kBatchOrders = 128;
    klt_affine_params ap{-1, 15, 15, 10, 10.f, 0.02f, 1.5f};      // klt.py:67-73 defaults
    klt_fb_params fbp{0, 1.0f};                                    // forward-backward check (klt_set_fb_params)
    klt_light_params lightp{0};                                    // gain / bias tracking (klt_set_light_params); 0 = off
    int light_path = 0;                                            // klt_track_light_path: kernel of the last lighting launch (0: none yet)
    SentTable<QualityPair> quality_table;                          // batched quality launches (klt_track_quality_batch_async)
    // the consensus checks (api_consensus.hip), in the order motion model (klt_set_model_params, klt_motion_check*), epipolar
    // (klt_set_epipolar_params, klt_epipolar_check*), homography (klt_set_homography_params, klt_homography_check*): each with scratch
    // and a pair table of its own, so that all three may be on in one context
    ConsensusState consensus[3] = {{{0, 0, 0, 256, 0u, 8, 1.0f, 1.0f}}, {{0, 0, 0, 512, 0u, 16, 1.0f, 0.f}}, {{0, 0, 0, 256, 0u, 8, 1.0f, 0.f}}};
    // crowding check (klt_set_crowd_params, klt_crowd_check*): scratch and list table of its own
    klt_crowd_params crowdp{0, 0, 0, 1};
    int crowd_path = 0;                                            // klt_crowd_check_path
    unsigned char *crowd_scratch = nullptr;
    size_t crowd_scratch_cap = 0;
    const int *crowd_rounds = nullptr;                             // in crowd_scratch: the last launch's round count (klt_crowd_check_rounds)
    SentTable<CrowdPair> crowd_table;                              // klt_crowd_check_batch_async
    // descriptors and their matcher (api_describe.hip): the parameters, the pattern in device memory (sent with the first describe
    // launch), the partial results of a match's ranges (forward, then backward) and the cut of the last match (0: none yet)
    klt_descriptor_params descp{1};
    klt_match_params matchp{64, 4, 5, 1, 0};
    int8_t *desc_pattern = nullptr;
    int4 *match_part = nullptr;
    size_t match_part_cap = 0;
    int match_splits = 0;                                          // klt_match_path
    // track identities (api_reacquire.hip): the parameters; one allocation made by the begin call (bank, counters, the dense fresh list,
    // the two sets of nearest-neighbour results) for the begin's n and capacity; the step counter; which of the two descriptor buffers
    // (kFbReacqDesc) holds P; the launches of the last begin / step (klt_reacquire_path)
    klt_reacquire_params reacqp{1024, 30, 64, 4, 5, 24};
    unsigned char *reacq_mem = nullptr;
    size_t reacq_mem_cap = 0;
    int reacq_n = -1, reacq_capacity = 0, reacq_k = 0, reacq_cur = 0, reacq_path = 0;      // reacq_n < 0: no sequence begun
    std::vector<AffState> aff;
    int select_aff_state = -1;
    int *placed_d = nullptr;
    const float *last_sel[3] = {nullptr, nullptr, nullptr};
    int sel_nc = 0, sel_nr = 0, sel_nx = 0, sel_ny = 0, sel_npow2 = 0;
    bool sel_valmap = false;          // the last selection wrote the eigenvalue map (one that used prepared scores did not)
    unsigned long long *stats_d = nullptr;
    bool collect_stats = false;
    bool use_fused = true;            // LDS-tiled fused kernels (pyramid_kernels.hip); off = generic two-pass kernels
    // timing
    bool timing = false;
    bool timing_stamps = false;               // klt_timing_enable(ctx, 2): single-launch kernel families are timed by their dispatch timestamps
    std::vector<Timed> pending;
    std::vector<hipEvent_t> pool;
    double acc_ms[F_COUNT] = {0}, acc_bytes[F_COUNT] = {0};
    unsigned acc_n[F_COUNT] = {0};
    unsigned acc_unstamped[F_COUNT] = {0};    // timing mode 2: scopes of a family whose launch did not go through klt_launch (nothing measured)
    // experiment (tools/graph_frame_probe.py, profiles/README.md "HIP graphs"): one frame's launch set captured into a HIP graph and replayed
    bool capturing = false;                   // the streams are being captured: nothing may synchronise or allocate
    hipGraphExec_t probe_graph = nullptr;
    int fail_alloc_in = -1;                   // KLT_OPT_FAIL_ALLOC_AFTER (test hook): >= 0 counts allocations down, the one that finds 0 fails
};

namespace kltapi {

// the 8-bit frame a slot holds as it came: the caller's device memory (adopted) or the slot's own raw buffer
inline const uint8_t *frame8(const Slot *s) { return s->u8_ext ? s->u8_ext : s->raw.u8; }
// the slot's 8-bit frame behind the stages of the chain up to and including `upto` that are switched on (api_frames.hip: the chain)
const uint8_t *ingest_output(const klt_ctx *c, const Slot *s, IngestStage upto);
// the 8-bit frame a slot's readers take: the output of the whole chain (ensure_ingested has made it)
inline const uint8_t *raw8(const klt_ctx *c, const Slot *s) { return ingest_output(c, s, INGEST_EQUALIZE); }

int fail(klt_ctx *c, int code, const std::string &msg);      // sets the context's message, returns `code`

#define HIPCHK(c, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail((c), KLT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));     \
    } while (0)

// Every device / pinned-host allocation of the library goes through these two (api_context.hip).  Out of memory is an ANSWER, not a device
// error: KLT_ERR_NOMEM with the size that was asked for, the pointer left null, and the runtime's sticky last-error cleared -- otherwise
// the next HIPCHK(c, hipGetLastError()) behind a launch would report a stale out-of-memory after the caller has already dealt with it.
int dev_alloc(klt_ctx *c, void **p, size_t bytes, const char *what);
int host_alloc(klt_ctx *c, void **p, size_t bytes, const char *what);
#define DEVALLOC(c, ptr, bytes)                                                                       \
    do {                                                                                             \
        if (int rc_ = kltapi::dev_alloc((c), (void **)&(ptr), (bytes), #ptr)) return rc_;            \
    } while (0)

struct TimerScope {
    klt_ctx *c;
    Timed t;
    bool on;
    hipStream_t st;
    bool stamps = false;
    TimerScope(klt_ctx *c_, int fam, double bytes, hipStream_t st_ = nullptr) : c(c_), on(c_->timing), st(st_ ? st_ : c_->work)
    {
        if (!on) return;
        t.fam = fam;
        t.bytes = bytes;
        for (hipEvent_t *e : {&t.a, &t.b}) {
            if (!c->pool.empty()) { *e = c->pool.back(); c->pool.pop_back(); }
            else if (hipEventCreate(e) != hipSuccess) { on = false; return; }
        }
        // families whose scope holds ONE launch that goes through klt_launch (the order kernel in front of a tracker and the threshold
        // kernel behind the eigenvalue pass do not): timed by that dispatch's own timestamps.  Scopes with several launches keep the pair
        stamps = c->timing_stamps && (fam == F_SMOOTH_GRAD || fam == F_PYR_REDUCE || fam == F_GRAD || fam == F_TRACK || fam == F_AFFINE || fam == F_CROWD_PREPARE || fam == F_CROWD ||
                                      fam == F_SAT_ROWS || fam == F_SAT_COLS || fam == F_EIGEN || fam == F_EQ_LUT || fam == F_EQ_APPLY || fam == F_REMAP || fam == F_DESCRIBE || fam == F_MATCH || fam == F_MATCH_RESOLVE ||
                                      fam == F_REACQ_CLASSIFY || fam == F_REACQ_BANK || fam == F_REACQ_FRESH || fam == F_REACQ_ASSIGN);
        if (stamps) { g_klt_stamp_start = t.a; g_klt_stamp_stop = t.b; }      // filled by the launch itself (klt_launch)
        else hipEventRecord(t.a, st);
    }
    ~TimerScope()
    {
        if (!on) return;
        if (stamps) {
            if (g_klt_stamp_start) {                 // no launch took them (an error path, or a launcher that does not go through
                c->acc_unstamped[t.fam]++;           // klt_launch): nothing was measured -- counted, klt_timing_read says so
                g_klt_stamp_start = g_klt_stamp_stop = nullptr;
                c->pool.push_back(t.a); c->pool.push_back(t.b);
                return;
            }
        } else {
            hipEventRecord(t.b, st);
        }
        c->pending.push_back(t);
    }
};

// whoever points c->work at the build stream holds one of these: the helpers enqueue on the main stream again on every way out
struct WorkScope {
    klt_ctx *c;
    ~WorkScope() { c->work = c->stream; }
};

// ---- api_context.hip
int drain_timers(klt_ctx *c);
int sync_all(klt_ctx *c);
int ensure_tmp(klt_ctx *c, size_t pixels);
int ensure_h1(klt_ctx *c, size_t floats);
int ensure_cimg(klt_ctx *c, size_t floats);
int get_slot(klt_ctx *c, int slot, Slot **out, bool create);
int get_fb(klt_ctx *c, int fb, int n, FeatBuf **out);
int fresh_event(klt_ctx *c, hipEvent_t *out, uint64_t *serial = nullptr);
bool event_live(const klt_ctx *c, uint64_t serial);
int wait_upload(klt_ctx *c, Slot *s, hipStream_t consumer);
int mark_consumed(klt_ctx *c, Slot *const *slots, int n, hipStream_t reader);
int mark_read(klt_ctx *c, Slot *const *slots, int n);
int wait_built(klt_ctx *c, Slot *s);
int check_ready(klt_ctx *c);

template <typename T>
int ensure(klt_ctx *c, T *&ptr, size_t &cap, size_t want)
{
    if (want <= cap && ptr) return 0;
    if (c->capturing) return fail(c, KLT_ERR_STATE, "a buffer would have to grow during a stream capture");
    if (ptr) { if (int rc = sync_all(c)) return rc; HIPCHK(c, hipFree(ptr)); ptr = nullptr; cap = 0; }
    DEVALLOC(c, ptr, want * sizeof(T));
    cap = want;
    return 0;
}

// The table goes up only when it differs from the one the device holds (pageable source: the runtime stages it before returning; stream
// order protects the launch that read the replaced table); *dev = where the launch finds it
template <class Desc>
int send_if_changed(klt_ctx *c, SentTable<Desc> &t, const std::vector<Desc> &table, const Desc **dev)
{
    if (t.host.size() != table.size() || std::memcmp(t.host.data(), table.data(), table.size() * sizeof(Desc)) != 0) {
        t.host.clear();                                      // (nothing is known of the device's copy until the new one is enqueued)
        if (int rc = ensure(c, t.dev, t.cap, table.size())) return rc;
        HIPCHK(c, hipMemcpyAsync(t.dev, table.data(), table.size() * sizeof(Desc), hipMemcpyHostToDevice, c->stream));
        t.host = table;
    }
    *dev = t.dev;
    return 0;
}

inline int mark_read_pair(klt_ctx *c, Slot *s1, Slot *s2)
{
    Slot *both[2] = {s1, s2};
    return mark_read(c, both, 2);
}

// ---- feature buffers as the launches look at them
// "buffer fb holds n records": an index of the context's table whose entry reaches n records ...
inline bool fb_holds(const klt_ctx *c, int fb, int n) { return fb >= 0 && (size_t)fb < c->fbs.size() && c->fbs[fb].cap >= n; }
// ... and has memory.  The two differ for n == 0 alone (an index below a used one that never got memory: no records, and none missing):
// the tracker's input lists, downloads and collectives ask the first, every other launch that reads a list the second
inline bool fb_holds_records(const klt_ctx *c, int fb, int n) { return fb_holds(c, fb, n) && c->fbs[fb].d; }

// KLT_ERR_STATE unless each of the launch's lists holds n records (in memory, unless the caller is the tracker)
inline int lists_set(klt_ctx *c, std::initializer_list<int> lists, int n, bool in_memory = true)
{
    for (int fb : lists)
        if (!(in_memory ? fb_holds_records(c, fb, n) : fb_holds(c, fb, n))) return fail(c, KLT_ERR_STATE, "input feature buffer not set");
    return 0;
}

// A launch's private record buffer (fb_guess, fb_quality, fb_model) holds records of its own.  By index, before the device or a slot is
// touched: a feature-buffer index that is none of `others` (an entry of -1 stands for no buffer) ...
inline int own_index(klt_ctx *c, int fb, std::initializer_list<int> others, const char *not_a_buffer, const char *not_distinct)
{
    if (fb < 0 || fb > 65535) return fail(c, KLT_ERR_ARG, not_a_buffer);
    for (int other : others)
        if (fb == other) return fail(c, KLT_ERR_ARG, not_distinct);
    return 0;
}
// ... and by address, once the launch's lists are known to exist: a view can be a second name of the same records (a buffer that does
// not exist yet is nobody's second name).  get_fb of the private buffer comes after both: a refused call allocates nothing
inline int own_records(klt_ctx *c, int fb, std::initializer_list<int> others, const char *not_distinct)
{
    if (!fb_holds_records(c, fb, 0)) return 0;
    for (int other : others)
        if (fb_holds_records(c, other, 0) && c->fbs[fb].d == c->fbs[other].d) return fail(c, KLT_ERR_ARG, not_distinct);
    return 0;
}

// ---- api_frames.hip
// (kMaxFramePixels, the bound on a frame: ingest_rule.h)
void make_taps(const double *k, int n, Taps &t);
int upload_raw(klt_ctx *c, int slot, const void *px, int ncols, int nrows, int pitch, int kind);
int layout_pyramid(klt_ctx *c, Slot *s);
int enqueue_smooth_raw(klt_ctx *c, Slot *s, float *dst);
int enqueue_gradients(klt_ctx *c, const float *img, int nc, int nr, float *rec);      // compact image -> pixel records
bool fused_smooth_ok(const klt_ctx *c);
bool fused_grad_ok(const klt_ctx *c);
int enqueue_fused_smooth_grad(klt_ctx *c, int batch, const void *const *raw, int raw_kind, float *const *rec,
                              float *const *cimg, int nc, int nr, const L0Plan &plan);
L0Plan plan_l0(const klt_ctx *c, int batch, int kind, int nc, int nr, bool uniform = true, bool want_hred = false, bool want_lean = false);
int enqueue_fused_grad(klt_ctx *c, int batch, const float *const *img, float *const *rec, int nc, int nr, bool u8_input = false);
int build_pyramids_batch(klt_ctx *c, const int *slot_ids, int n);
// The ingest chain in front of every reader of a slot's raw frame: the 8-bit frames of these slots that have no valid copy of a stage
// that is switched on get one, enqueued on `st` (behind the frames' uploads: the caller has waited for them there), remap before CLAHE,
// the slots of one frame size in the same launches, KLT_MAX_BATCH at a time.  Every refusal of every stage comes before the first
// allocation, every allocation before the first launch: a call that fails has enqueued nothing and leaves the slots' copies and flags as
// they were.  KLT_ERR_STATE for an f32 slot or a launch during a stream capture, KLT_ERR_ARG for a frame a stage does not take,
// KLT_ERR_NOMEM.  of_build: klt_remap_path / klt_equalize_path become 1 for the stages that launch (the build has cleared both)
int ensure_ingested(klt_ctx *c, Slot *const *slots, int n, hipStream_t st, bool of_build = false);
// ... and the refusals of one slot that hold whether or not anything would be launched (the build asks in front of layout_pyramid)
int ingest_refusal(klt_ctx *c, const Slot *s);
// Something changed at `stage` of the chain: the copies of `s` from there on are stale (a new frame: everything, the pyramids included;
// a new map: the remapped and the equalised copy; new equalisation parameters: the equalised copy)
void void_copies_from(Slot &s, IngestStage stage);
// KLT_OPT_L0_LAZY_GRAD: whoever reads lv[0].img / .gx / .gy of a built slot calls this first.  The records of a lean slot are made from its
// compact image by the gradient launch of the levels >= 1, on the main stream behind the slot's build (wait_built); a caller that
// enqueues on the build stream is ordered behind it.  `asked` (every reader but the tracker's own fallback): the slot's next build is full.
int ensure_level0_records(klt_ctx *c, Slot *s, bool asked = true);
int ensure_level0_records(klt_ctx *c, Slot *const *slots, int n, bool asked = true);      // ... of several slots: one launch per KLT_MAX_BATCH slots of a size
bool merged_grad_ok(const klt_ctx *c);                       // 7-tap Gaussian / derivative gradient filters (what the specialised kernels take)
int download_plane(klt_ctx *c, const float *src, int stride, size_t cnt, float *dst);      // every stride-th float of a device plane to the host

// ---- api_track.hip
// both slots hold built pyramids of one geometry (and the main stream waits for their builds); their level-0 records are there
// (ensure_level0_records) unless the caller has a lazy form and looks after that itself (lazy_ok)
int check_pair(klt_ctx *c, int slot1, int slot2, Slot **p1, Slot **p2, bool lazy_ok = false);
void level_planes(const Slot *s1, const Slot *s2, int l, const float *&i1, const float *&gx1, const float *&gy1, const float *&i2,
                  const float *&gx2, const float *&gy2);                     // the six planes of level l of a frame pair
int refuse_with_light(klt_ctx *c, const char *what);                         // KLT_ERR_STATE while gain / bias tracking is switched on
int count_live(const klt_feat *f, int n);
// a batched launch on frame pairs: its argument test (`columns`: the arrays of the call, none may be null), and pair by pair -- so that
// the order of refusals stays pair 0's slots, pair 0's lists, pair 1's slots, ... -- the pair's slots (check_pair) appended to `used`
// and held against the first pair's frame size (and level count, if `same_levels`)
int batch_arguments(klt_ctx *c, std::initializer_list<const int *> columns, int npairs, int n);
int batch_pair(klt_ctx *c, int slot1, int slot2, bool same_levels, std::vector<Slot *> &used, bool lazy_ok = false);

// ---- api_describe.hip
// klt_describe_async in its two halves, for a caller with allocations of its own to place between them (api_reacquire.hip): every
// refusal (nothing is allocated or enqueued; *s = the slot), then the allocations followed by the launch
int describe_refusals(klt_ctx *c, int slot, int fb_in, int fb_desc, int n, Slot **s);
int describe_enqueue(klt_ctx *c, Slot *s, int fb_in, int fb_desc, int n);
bool match_params_ok(const klt_match_params &p);             // what klt_set_match_params takes

// ---- api_select.hip
// the three summed-area tables of a gradient pair (goodFeaturesUtils.pyx:49-51); rows_only: the column pass is left to the caller
int enqueue_sat(klt_ctx *c, hipStream_t st, const float *gx, const float *gy, float *sat, int nc, int nr, bool rows_only = false);

}  // namespace kltapi
