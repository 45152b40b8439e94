// api_select.hip -- selection (goodFeaturesUtils.pyx:17-73, selectGoodFeatures.py:45-135, :141-261): scores prepared ahead of a
// replacement, the two-halves protocol around the host's look at the outcome (klt_select_begin_async / klt_select_finish), the walk over
// a given candidate list, and the hooks the parity tests inspect a selection through.
#include "klt_context.h"

namespace kltapi {
// summed-area tables of the gradient products (goodFeaturesUtils.pyx:49-51): step-synchronous wavefront pipelines (sat_pipeline.hip)
// where whole aligned quads can be moved, else the barrier-coupled kernels of select_kernels.hip

// the tables' column pass: the pipeline kernel where it takes the geometry (a positive code is a device error), else the barrier kernel
static int enqueue_sat_cols(klt_ctx *c, hipStream_t st, float *sat, int nc, int nr)
{
    TimerScope t(c, F_SAT_COLS, (double)nc * nr * 24);
    const int e = c->sat_variant == 1 ? launch_sat_cols_pipe(st, sat, nc, nr) : -1;
    if (e > 0) return fail(c, KLT_ERR_DEVICE, hipGetErrorString((hipError_t)e));
    if (e < 0) launch_sat_cols(st, sat, nc, nr);
    c->score_cols_path = e < 0 ? KLT_SCORE_BARRIER : KLT_SCORE_PIPELINE;        // klt_select_score_path
    return 0;
}

int enqueue_sat(klt_ctx *c, hipStream_t st, const float *gx, const float *gy, float *sat, int nc, int nr, bool rows_only)
{
    { TimerScope t(c, F_SAT_ROWS, (double)nc * nr * (8 + 12));
      const int e = c->sat_variant == 1 ? launch_sat_rows_pipe(st, gx, gy, sat, nc, nr) : -1;
      if (e > 0) return fail(c, KLT_ERR_DEVICE, hipGetErrorString((hipError_t)e));
      if (e < 0) launch_sat_rows(st, gx, gy, sat, nc, nr);
      c->score_rows_path = e < 0 ? KLT_SCORE_BARRIER : KLT_SCORE_PIPELINE; }    // klt_select_score_path
    return rows_only ? 0 : enqueue_sat_cols(c, st, sat, nc, nr);
}

}  // namespace kltapi

namespace {
// smallest power of two >= x, at least 2048 (the sort takes whole 2048-key chunks)
long long pow2_at_least_2048(long long x) { long long p = 2048; while (p < x) p <<= 1; return p; }

// the list as select_job_start / serial_selection found it, back from the snapshot
int restore_list(klt_ctx *c, klt_feat *fl, int n)
{
    HIPCHK(c, hipMemcpyAsync(fl, c->fl_snapshot, (size_t)n * sizeof(klt_feat), hipMemcpyDefault /* the list may be pinned host memory (klt_featbuf_map_host) */, c->stream));
    return 0;
}

// ---- per-cell quota (klt_set_select_grid)
// the quota's arguments on an nc x nr frame and its buffer (klt_context.h), not cleared
int make_quota_args(klt_ctx *c, int nc, int nr, QuotaArgs &qa)
{
    const klt_select_grid &g = c->sel_grid;
    const long long gw = ((long long)nc + g.cell_width - 1) / g.cell_width, gh = ((long long)nr + g.cell_height - 1) / g.cell_height;
    const size_t cells = (size_t)(gw * gh);                        // at most one per pixel
    if (int rc = ensure(c, c->quota_buf, c->quota_buf_cap, 3 * cells + (cells + 1) / 2 + 1)) return rc;
    qa.live = (unsigned *)(c->quota_buf + 3 * cells);
    qa.cw = g.cell_width; qa.ch = g.cell_height; qa.gw = (int)gw; qa.q = g.max_per_cell; qa.cells = (int)cells;
    qa.cw_magic = g.cell_width >= 65536 ? 0u : klt_div_magic((unsigned)g.cell_width);
    qa.ch_magic = g.cell_height >= 65536 ? 0u : klt_div_magic((unsigned)g.cell_height);
    return 0;
}
unsigned *quota_nkept(const QuotaArgs &qa) { return qa.live + qa.cells; }

// live(cell) of list `fl` in stream order, in front of the filter or the walk: a repeat comes through here again, with the list back from
// its snapshot.  rounds: the filter's planes and its count are cleared as well.
int enqueue_quota_live(klt_ctx *c, const QuotaArgs &qa, bool rounds, const klt_feat *fl, int n, bool overwrite_all, int nc, int nr)
{
    if (rounds) HIPCHK(c, hipMemsetAsync(c->quota_buf, 0, 3 * (size_t)qa.cells * sizeof(unsigned long long) + ((size_t)qa.cells + 1) * sizeof(unsigned), c->stream));
    else HIPCHK(c, hipMemsetAsync(qa.live, 0, (size_t)qa.cells * sizeof(unsigned), c->stream));
    if (!overwrite_all) launch_quota_live(c->stream, fl, n, nc, nr, qa);      // KLT_SELECTING_ALL: every slot is free, no feature counts
    return 0;
}

// the greedy walk over na.keys: the cell grid cleared first where it lives in global memory, the live counts first where there is a quota
int enqueue_walk(klt_ctx *c, const NmsArgs &na, const QuotaArgs *qa, int ncols, int nrows)
{
    if (!na.grid_in_lds) HIPCHK(c, hipMemsetAsync(c->grid, 0, (size_t)na.gw * na.gh * sizeof(uint32_t), c->stream));
    TimerScope t(c, F_NMS, (double)na.nfeat * 16);
    if (qa)
        if (int rc = enqueue_quota_live(c, *qa, false, na.fl, na.nfeat, na.overwrite_all != 0, ncols, nrows)) return rc;
    if (const int e = launch_nms(c->stream, na, qa)) return fail(c, KLT_ERR_DEVICE, std::string("nms launch: ") + hipGetErrorString((hipError_t)e));
    return 0;
}

// start of an attempt: free slots + snapshot of the list, scores / histogram / cut (attempt 0) or "every candidate" (attempt 1), tile lists
int select_job_start(klt_ctx *c, SelectJob &j)
{
    j.filtered = j.prefilter && j.attempt == 0;
    SelectArgs &sa = j.sa;
    if (j.attempt == 0) {
        launch_mis_prepare(c->stream, j.fl, j.n, j.pa.overwrite_all, j.pa.slots, j.nfill_d, c->fl_snapshot, j.zero_from, j.zero_n);
        if (j.filtered) { sa.hist = j.hist_d; sa.ticket = j.ticket_d; sa.info = j.info_d; sa.hist_target = (unsigned)((j.target + 3) / 4); }
        if (j.filtered && j.mode == KLT_REPLACING_SOME) {
            // only the lost features' slots are filled and the live features' squares are not scored at all: 64 candidates per
            // LOST feature (at least 4096) instead of 64 per list entry -- most of a frame's candidates never enter the passes.
            // (cfg-5, 50-95 lost of 20000 per frame: a floor of 65536 / 16384 / 4096 / 1024 candidates reads 0.424 / 0.387 /
            // 0.365 / 0.364 ms per frame; too tight a cut only costs the repeat below, never the result)
            sa.hist_target = 4096 / 4 * j.cut_scale; sa.hist_slots = j.nfill_d; sa.hist_per_slot = 64 / 4 * j.cut_scale;
        }
        if (j.pre) {
            // scored ahead of time without the seed map: histogram of the keys outside it here, the mask itself in mis_init
            sa.keys = j.pre->keys;
            TimerScope t(c, F_EIGEN, (double)j.ncand * 2);
            launch_mask_hist(c->stream, sa);
        } else {
            // SURVEY 8(d) [score]: the three table planes once + eigenvalue and key per candidate
            TimerScope t(c, F_EIGEN, 12.0 * sa.ncols * sa.nrows + (double)j.ncand * (4 + 8));
            launch_eigen_hist(c->stream, sa);
        }
    } else {
        launch_zero_words(c->stream, j.zero_from, j.zero_n);      // threshold bin 0: every candidate
        j.ma.sparse = 0;
    }
    if (!j.by_rank) HIPCHK(c, hipMemsetAsync(c->keys2, 0, (size_t)j.np2 * sizeof(unsigned long long), c->stream));
    j.round = 0;
    TimerScope t(c, F_NMS, (double)j.ncand * 12);
    launch_mis_init(c->stream, j.ma);
    return 0;
}

// a batch of passes, then the accepted candidates ranked and placed, and the few words the host looks at written to pinned memory
int select_job_rounds(klt_ctx *c, SelectJob &j)
{
    {
        TimerScope t(c, F_NMS, (double)j.n * 16);
        for (int r = 0; r < j.rounds_per_look; r++, j.round++, j.passes++)
            if (const int e = launch_mis_round(c->stream, j.ma, j.round))
                return fail(c, KLT_ERR_DEVICE, std::string("minimum-distance pass: ") + hipGetErrorString((hipError_t)e));
    }
    j.look = j.round < 64 ? j.round : 64;                        // the last `look` passes
    const unsigned *rem_d = j.ma.remaining + j.round - j.look;
    launch_mis_compact(c->stream, j.ma, c->keys2, j.acc_count_d);
    if (j.by_rank) {
        TimerScope t(c, F_NMS, (double)j.n * 16 + (j.quota ? (double)j.bound * 8 * (j.qa.q + 1) : 0.0));
        if (j.quota) {
            // the accepted candidates beyond their cell's room leave keys2 before the rest is ranked and placed
            if (int rc = enqueue_quota_live(c, j.qa, true, j.fl, j.n, j.pa.overwrite_all != 0, j.ncols, j.nrows)) return rc;
            launch_quota_filter(c->stream, c->keys2, j.acc_count_d, (int)j.bound, j.qa, c->quota_buf, j.qa.cells, quota_nkept(j.qa));
        }
        launch_mis_place(c->stream, j.pa, j.acc_count_d, j.quota ? quota_nkept(j.qa) : nullptr, j.rank_d, j.nfill_d, (int)j.bound, c->readback,
                         rem_d, j.look, j.info_d);
    } else {
        { TimerScope t(c, F_SORT, (double)j.np2 * 16); launch_sort_desc(c->stream, c->keys2, (int)j.np2); }
        if (int rc = enqueue_walk(c, j.pa, j.quota ? &j.qa : nullptr, j.ncols, j.nrows)) return rc;      // (j.pa's cell grid is one word in LDS)
        launch_mis_results(c->stream, c->readback, rem_d, j.look, j.info_d, c->placed_d);
    }
    // the host's look waits for THIS point of the stream, not for the stream: a caller may enqueue work that only reads the list (the next
    // frame's tracker) between the two halves, and the GPU keeps it queued while the host looks and enqueues the next selection
    if (!c->ev_sel) HIPCHK(c, hipEventCreateWithFlags(&c->ev_sel, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_sel, c->stream));
    return 0;
}

// the host's look at the outcome, and whatever it asks for; returns when the selection is complete
int select_job_finish(klt_ctx *c, SelectJob &j)
{
    const unsigned *const rem = c->readback, *const info = c->readback + 64, *const res = c->readback + 72;
    int looks = 0;                       // > 1: the list was rewritten after the launches of klt_select_begin_async had run
    for (;;) {
        HIPCHK(c, hipEventSynchronize(c->ev_sel));
        looks++;
        if (rem[j.look - 1] != 0u) {
            // a dependency chain longer than the passes run so far: put the list back and keep going
            if (j.round + j.rounds_per_look > SelectJob::kMaxRounds) return fail(c, KLT_ERR_DEVICE, "minimum-distance passes did not settle");
            if (int rc = restore_list(c, j.fl, j.n)) return rc;
            if (j.by_rank) launch_zero_words(c->stream, j.rank_d, (size_t)j.bound);
            else HIPCHK(c, hipMemsetAsync(c->keys2, 0, (size_t)j.np2 * sizeof(unsigned long long), c->stream));
            if (int rc = select_job_rounds(c, j)) return rc;
            continue;
        }
        int needed = j.look;                                         // learn how many passes were needed
        while (needed > 1 && rem[needed - 2] == 0u) needed--;
        needed += j.round - j.look;
        // replacement runs frame after frame: one spare pass, because a frame that needs one pass more than the last
        // one costs a host round trip and another batch of passes, an idle pass 2-5 us
        if (j.mode == KLT_REPLACING_SOME) needed += 1;
        c->mis_rounds_hint = needed < 2 ? 2 : (needed > 32 ? 32 : needed);
        c->sorted_keys = j.by_rank ? nullptr : c->keys2; c->sorted_count = j.by_rank ? 0 : (int)j.np2;
        // ran out of accepted candidates although the prefilter dropped some: repeat with every candidate.  info[3] is mis_init_kernel's
        // word "the threshold bin kept a valid key out" -- exact, where info[1] and info[2] count the histogram's sample only (a sample
        // that lies wholly at or above the bin says nothing of the keys it did not see)
        if (j.filtered && res[1] && info[3]) {
            if (int rc = restore_list(c, j.fl, j.n)) return rc;
            j.attempt = 1;
            if (int rc = select_job_start(c, j)) return rc;
            if (int rc = select_job_rounds(c, j)) return rc;
            continue;
        }
        break;
    }
    if (j.pre) j.pre->gen = 0;                                       // a score set is used once
    HIPCHK(c, hipGetLastError());
    // klt_select_pick_path
    c->pick = klt_select_pick{1, j.by_rank ? 1 : 2, j.prefilter ? 1 : 0, j.attempt + 1, j.passes, looks, j.ma.R == 9 ? 9 : 0,
                              (int32_t)mis_pass_lds(j.ma), j.pa.grid_in_lds ? 0 : 1, j.ma.sparse};
    return looks > 1 ? 1 : KLT_OK;
}

// borders / half-windows as ScanImageForGoodFeatures receives them: Python floats truncated to C ints
// (selectGoodFeatures.py:168-169, :215-221, goodFeaturesUtils.pyx:35-37)
struct SelGeom { int bx, by, hw, hh, step, nx, ny; long long ncand, npow2; };
int select_geometry(klt_ctx *c, int nc, int nr, SelGeom *g)
{
    const klt_params &p = c->p;
    double bxd = p.borderx, byd = p.bordery;
    if (bxd < p.window_width / 2.0) bxd = p.window_width / 2.0;
    if (byd < p.window_height / 2.0) byd = p.window_height / 2.0;
    g->bx = (int)bxd; g->by = (int)byd; g->hw = p.window_width / 2; g->hh = p.window_height / 2;
    g->step = p.nSkippedPixels + 1;
    if (g->bx - g->hw - 1 < 0 || g->by - g->hh - 1 < 0)
        return fail(c, KLT_ERR_ARG, "border must be at least window/2 + 1 (the reference reads outside the image otherwise)");
    g->nx = (nc - g->bx > g->bx) ? (nc - 2 * g->bx + g->step - 1) / g->step : 0;
    g->ny = (nr - g->by > g->by) ? (nr - 2 * g->by + g->step - 1) / g->step : 0;
    g->ncand = (long long)g->nx * g->ny;
    g->npow2 = pow2_at_least_2048(g->ncand);
    if (g->npow2 > (1LL << 30)) return fail(c, KLT_ERR_ARG, "too many candidates");
    return 0;
}

double select_min_eig(const klt_params &p) { return p.min_eigenvalue < 1 ? 1.0 : p.min_eigenvalue; }      // selectGoodFeatures.py:53

// the frame, the candidate lattice and the eigenvalue floor of a zeroed SelectArgs; the buffers are the caller's
void fill_select_geometry(SelectArgs &sa, int nc, int nr, const SelGeom &g, double min_eig)
{
    sa.min_eig = min_eig;
    sa.ncols = nc; sa.nrows = nr; sa.bx = g.bx; sa.by = g.by; sa.step = g.step; sa.nx = g.nx; sa.ny = g.ny;
    sa.hw = g.hw; sa.hh = g.hh; sa.npow2 = (int)g.npow2;
}

// the greedy walk's arguments over list `fl` with exclusion distance d (mindist - 1) on an ncols x nrows frame: slot scratch and cell grid
// are there when this returns, the grid NOT cleared; keys, nkeys and aff_rec are the caller's
int make_nms_args(klt_ctx *c, klt_feat *fl, int n, bool overwrite_all, int d, int ncols, int nrows, NmsArgs &na)
{
    std::memset(&na, 0, sizeof(na));
    na.fl = fl; na.placed_out = c->placed_d;
    na.nfeat = n; na.overwrite_all = overwrite_all;
    na.d = d; na.cell = d >= 0 ? d + 1 : 1;
    na.cell_magic = na.cell == 1 ? 0u : klt_div_magic((unsigned)na.cell);
    if (int rc = ensure(c, c->nms_slots, c->nms_slots_cap, (size_t)n)) return rc;
    na.slots = c->nms_slots;
    na.gw = d >= 0 ? (ncols + na.cell - 1) / na.cell : 1;
    na.gh = d >= 0 ? (nrows + na.cell - 1) / na.cell : 1;
    na.grid_in_lds = (size_t)na.gw * na.gh * sizeof(uint32_t) <= 128 * 1024;     // + 12.4 KiB of static LDS in the kernel
    if (!na.grid_in_lds) {
        if (int rc = ensure(c, c->grid, c->grid_cap, (size_t)na.gw * na.gh)) return rc;
        na.grid_global = c->grid;
    }
    return 0;
}

// The counters of the parallel passes, one allocation: [tiles] list lengths | [kMaxRounds] "undecided left after pass r" | accepted count |
// workgroup ticket | [tiles] accepted per tile | 8192 histogram bins + 4 words of prefilter info | [bound] ranks (when ranking by counting)
struct MisCounters {
    size_t lists = 0, remaining, accepted, ticket, tile_accepted, hist, info, rank, total;      // where each part starts, in words
    MisCounters(int tiles, long long bound, bool by_rank)
        : remaining((size_t)tiles), accepted(remaining + SelectJob::kMaxRounds), ticket(accepted + 1), tile_accepted(ticket + 1),
          hist(tile_accepted + tiles), info(hist + 8192), rank(info + 4), total(rank + (by_rank ? (size_t)bound : 0)) {}
    size_t zero_from() const { return remaining; }      // an attempt starts with everything behind the list lengths zeroed
    size_t zero_n() const { return total - remaining; }
};

ScoreCache *find_scores(klt_ctx *c, const Slot *s, const SelGeom &g, double min_eig)
{
    if (!s->pyr_valid || !s->gen) return nullptr;
    for (auto &e : c->pre)
        if (e.gen == s->gen && e.nc == s->nc && e.nr == s->nr && e.bx == g.bx && e.by == g.by && e.hw == g.hw && e.hh == g.hh &&
            e.step == g.step && e.nx == g.nx && e.ny == g.ny && e.min_eig == min_eig)
            return &e;
    return nullptr;
}

// ---- the steps of klt_select_begin_async, in the order it takes them
// leaves the four scratch planes of an N-pixel frame (all of them or none), the key buffer and the convolution scratch
int ensure_select_scratch(klt_ctx *c, size_t N, long long npow2)
{
    if (N > c->sel_cap) {
        if (c->sel_img) { if (int rc = sync_all(c)) return rc; hipFree(c->sel_img); hipFree(c->sel_rec); hipFree(c->sat); hipFree(c->valmap); }
        c->sel_img = c->sel_rec = c->sat = c->valmap = nullptr;
        c->sel_cap = 0;                                       // (nothing is held until all four planes are: a failure below frees what it got)
        int rc_alloc = dev_alloc(c, (void **)&c->sel_img, N * sizeof(float), "selection scratch: image");
        if (!rc_alloc) rc_alloc = dev_alloc(c, (void **)&c->sel_rec, KLT_PIX_STRIDE * N * sizeof(float), "selection scratch: pixel records");      // image, gradx, grady, like a slot's levels
        if (!rc_alloc) rc_alloc = dev_alloc(c, (void **)&c->sat, 3 * N * sizeof(float), "selection scratch: summed-area tables");
        if (!rc_alloc) rc_alloc = dev_alloc(c, (void **)&c->valmap, N * sizeof(float), "selection scratch: eigenvalue map");
        if (rc_alloc) {
            hipFree(c->sel_img); hipFree(c->sel_rec); hipFree(c->sat); hipFree(c->valmap);
            c->sel_img = c->sel_rec = c->sat = c->valmap = nullptr;
            return rc_alloc;
        }
        c->sel_cap = N;
    }
    if (int rc = ensure(c, c->keys, c->keys_cap, (size_t)npow2)) return rc;
    return ensure_tmp(c, N);
}

// leaves the image and gradient planes the selection scores, enqueued on the stream: the slot's level-0 pyramid reused
// (selectGoodFeatures.py:176-181) or computed afresh from the raw frame (:183-197)
int select_planes(klt_ctx *c, Slot *s, int use_pyramid, const float **img_out, const float **gx, const float **gy)
{
    const int nc = s->nc, nr = s->nr;
    const float *img = nullptr;
    if (use_pyramid) {
        if (!s->pyr_valid) return fail(c, KLT_ERR_STATE, "use_pyramid requested but the slot's pyramids are not built");
        if (int rc = wait_built(c, s)) return rc;
        if (int rc = ensure_level0_records(c, s)) return rc;
        *img_out = s->lv[0].img; *gx = s->lv[0].gx; *gy = s->lv[0].gy;
        return 0;
    }
    if (s->raw_kind == 0) return fail(c, KLT_ERR_STATE, "slot has no frame");
    if (int rc = wait_upload(c, s, c->stream)) return rc;
    if (int rc = wait_built(c, s)) return rc;              // a build of this slot may still read the raw frame's buffers
    if (int rc = ensure_ingested(c, &s, 1, c->stream)) return rc;      // the ingest stages: the readers below take the chain's output (raw8), made now where it is stale
    bool grads_done = false;
    if (c->p.smoothBeforeSelecting && fused_smooth_ok(c)) {
        const void *raw = s->raw_kind == 1 ? (const void *)raw8(c, s) : (const void *)rawf(s);
        if (int rc = enqueue_fused_smooth_grad(c, 1, &raw, s->raw_kind, &c->sel_rec, nullptr, nc, nr, plan_l0(c, 1, s->raw_kind == 1 ? 0 : 1, nc, nr)))
            return rc;
        grads_done = true;
    } else if (c->p.smoothBeforeSelecting) {
        enqueue_smooth_raw(c, s, c->sel_img);
        img = c->sel_img;
    } else if (s->raw_kind == 2) {
        img = rawf(s);
    } else {
        // u8 -> f32 with a 1-tap identity kernel is overkill; widen with a 1-tap correlate (exact)
        Taps one;
        std::memset(&one, 0, sizeof(one));
        one.n = 1; one.sym = 1; one.k[0] = 1.0;
        launch_hconv_u8(c->stream, raw8(c, s), nc, nr, c->sel_img, nullptr, nc, 1, 0, one, nullptr);
        img = c->sel_img;
    }
    if (!grads_done) {
        // the compact image (a raw f32 frame or sel_img) -> the records, image copied through
        if (fused_grad_ok(c)) { if (int rc = enqueue_fused_grad(c, 1, &img, &c->sel_rec, nc, nr)) return rc; }
        else enqueue_gradients(c, img, nc, nr, c->sel_rec);
    }
    *img_out = c->sel_rec; *gx = c->sel_rec + 1; *gy = c->sel_rec + 2;
    // the kernels above read the raw frame: the second-next asynchronous copy into this slot (its raw buffers alternate) waits
    return mark_consumed(c, &s, 1, c->stream);
}

// what a selection of n features in `mode` will do, decided from the geometry and the options alone; nothing is enqueued
struct SelPlan {
    int d, R;                     // mindist - 1; exclusion radius in candidate cells (-1: none)
    bool parallel_nms, prefilter;
    long long target;             // candidates the prefilter aims to keep
    int cut_scale;                // 1, or the factor a grid widens the cuts by
    double min_eig;
    ScoreCache *pre;              // scores prepared ahead of time that this selection uses, or null
};
SelPlan plan_selection(klt_ctx *c, const Slot *s, const SelGeom &g, int mode, int use_pyramid, int n)
{
    SelPlan pl;
    const int mindist = c->p.mindist < 0 ? 0 : c->p.mindist;          // selectGoodFeatures.py:241-243
    pl.d = mindist - 1;                                               // :61
    pl.R = pl.d >= 0 ? pl.d / g.step : -1;
    pl.parallel_nms = c->use_mis && g.ncand > 0 && mis_stage_bytes(pl.R) <= 120 * 1024;
    pl.target = 64LL * n;
    if (pl.target < 65536) pl.target = 65536;
    // under a grid (klt_set_select_grid) the walk turns candidates away, so a cut sized for "best first" runs out sooner and the repeat with
    // every candidate is likelier.  KLT_GRID_CUT_SCALE widens every cut of a selection under a grid by that factor; 1 (the default): the
    // figures of tools/grid_probe.py did not call for more.  Too tight a cut costs the repeat, never the result.
    static const int grid_cut_scale = getenv("KLT_GRID_CUT_SCALE") ? atoi(getenv("KLT_GRID_CUT_SCALE")) : 1;
    pl.cut_scale = c->sel_grid.cell_width > 0 && grid_cut_scale > 1 ? (grid_cut_scale > 64 ? 64 : grid_cut_scale) : 1;
    pl.target *= pl.cut_scale;
    pl.prefilter = c->use_topk && g.ncand > 262144 && pl.target < g.ncand / 2;
    pl.min_eig = select_min_eig(c->p);
    // scores prepared ahead of time (klt_select_prepare_async) are used by the replacement pass of the parallel path; everything else
    // computes them here
    pl.pre = nullptr;
    if (mode == KLT_REPLACING_SOME && use_pyramid && pl.parallel_nms && pl.prefilter && pl.d >= 0 && !c->score_override_n)
        pl.pre = find_scores(c, s, g, pl.min_eig);
    return pl;
}

struct Consume {                                           // a set is used once: the selection frees it when it is through with it
    ScoreCache *e;
    ~Consume() { if (e) e->gen = 0; }
};

// ---- the seed map: per-pixel "never a candidate" marks, read by the scoring kernels (eigen_key, mask_hist_kernel) and by mis_init.  It is
// stamped, not cleared: a pixel is blocked when it carries THIS selection's stamp.  One step begins the map, two steps fill it.

// Leaves a map for an nc x nr frame in which no pixel carries the stamp c->seed_stamp (a new one): allocated (whole 16-byte pieces, which
// fill_select_mask stores), cleared when it is new, when the frame size changed or when the stamps wrapped at 255.
int begin_seed_map(klt_ctx *c, int nc, int nr, const uint8_t **seed)
{
    const size_t N = (size_t)nc * nr, padded = (N + 15) & ~(size_t)15;
    const uint8_t *before = c->seedmap;
    if (int rc = ensure(c, c->seedmap, c->seed_cap, padded)) return rc;
    if (c->seedmap != before || c->seed_n != N || c->seed_stamp == 255) {       // new map, other frame size, or the stamps wrapped
        HIPCHK(c, hipMemsetAsync(c->seedmap, 0, padded, c->stream));
        c->seed_n = N;
        c->seed_stamp = 0;
    }
    c->seed_stamp++;
    *seed = c->seedmap;
    return 0;
}

// REPLACING_SOME: the squares of the live features are marked; the eigenvalue kernels skip marked pixels, so neither the
// scoring nor the minimum-distance stage ever sees them.
void fill_live_squares(klt_ctx *c, const klt_feat *fl, int n, int nc, int nr, int d)
{
    TimerScope t(c, F_SEED, (double)n * 16);
    launch_seed_fill(c->stream, fl, n, c->seedmap, nc, nr, d, c->seed_stamp);
}

// klt_set_select_mask*: the pixels whose mask byte is 0 are marked the same way.  The mask is read here, once per selection: a repeat inside
// klt_select_finish reuses the stamped map.
void fill_select_mask(klt_ctx *c, int nc, int nr)
{
    const size_t N = (size_t)nc * nr;
    TimerScope t(c, F_SEED, 2.0 * N);
    launch_seed_mask(c->stream, c->mask, c->seedmap, N, c->seed_stamp);
}

// a mask belongs to frames of one size: another one is the caller's mistake, found before anything is enqueued
int check_select_mask(klt_ctx *c, int nc, int nr)
{
    if (!c->mask || (c->mask_nc == nc && c->mask_nr == nr)) return 0;
    char msg[160];
    snprintf(msg, sizeof msg, "the selection mask is %d x %d, the slot's frame %d x %d (klt_set_select_mask)", c->mask_nc, c->mask_nr, nc, nr);
    return fail(c, KLT_ERR_ARG, msg);
}

// ---- parallel minimum distance (default): decide every candidate in a few passes, rank the accepted ones, and
// fill the free slots with the best of them (same result as the sorted serial walk below).  Leaves the first batch of passes
// enqueued and the job with the context, for klt_select_finish.
int begin_parallel_selection(klt_ctx *c, const SelPlan &pl, const SelectArgs &sa, const NmsArgs &na, int mode, Consume &consume,
                             const QuotaArgs *qa)
{
    const int nx = sa.nx, ny = sa.ny, R = pl.R, n = na.nfeat;
    const long long ncand = (long long)nx * ny;
    auto job = std::make_unique<SelectJob>();
    SelectJob &j = *job;
    // passes enqueued before the host looks at the outcome: what the previous selection needed (frames of a sequence
    // behave alike); an idle pass costs 5 us, a second look costs a host round trip
    j.rounds_per_look = c->mis_rounds_hint;
    const int tiles = mis_tiles(nx, ny);
    // two accepted candidates are more than R cells apart in x or in y: at most one per (R+1)x(R+1) block of cells
    j.bound = R < 0 ? ncand : (long long)((nx + R) / (R + 1)) * ((ny + R) / (R + 1));
    j.by_rank = j.bound <= 98304;                       // rank by counting; beyond that sort the accepted keys
    if (qa) {
        // the filter takes one launch per feature a cell may hold: beyond KLT_QUOTA_MAX_ROUNDS the accepted keys are sorted and walked
        j.quota = true; j.qa = *qa; j.ncols = sa.ncols; j.nrows = sa.nrows;
        if (qa->q > KLT_QUOTA_MAX_ROUNDS) j.by_rank = false;
        c->grid_path = j.by_rank ? 1 : 2;
    }
    j.np2 = pow2_at_least_2048(j.bound);
    const MisCounters cnt(tiles, j.bound, j.by_rank);
    const int tile_cap = mis_tile_capacity(R);
    if (int rc = ensure(c, c->keys2, c->keys2_cap, (size_t)(j.np2 > sa.npow2 ? j.np2 : sa.npow2))) return rc;
    if (int rc = ensure(c, c->mis_st, c->mis_st_cap, (size_t)ncand)) return rc;
    if (int rc = ensure(c, c->mis_list, c->mis_list_cap, (size_t)tiles * 1024)) return rc;
    if (int rc = ensure(c, c->mis_cnt, c->mis_cnt_cap, cnt.total)) return rc;
    if (int rc = ensure(c, c->mis_tile_keys, c->mis_tile_keys_cap, (size_t)tiles * tile_cap)) return rc;
    if (int rc = ensure(c, c->fl_snapshot, c->fl_snapshot_cap, (size_t)n)) return rc;
    // results come back through pinned host memory the kernels write to directly
    if (!c->readback) {
        void *hp = nullptr;
        if (int rc = host_alloc(c, &hp, 128 * sizeof(unsigned), "selection read-back words")) return rc;
        c->readback = (unsigned *)hp;
        c->pinned.push_back(hp);
    }
    unsigned *const base = c->mis_cnt;
    j.fl = na.fl; j.n = n; j.ncand = ncand; j.mode = mode; j.prefilter = pl.prefilter; j.target = pl.target; j.cut_scale = pl.cut_scale; j.pre = pl.pre;
    j.zero_from = base + cnt.zero_from(); j.zero_n = cnt.zero_n();
    j.hist_d = base + cnt.hist; j.ticket_d = base + cnt.ticket; j.info_d = base + cnt.info; j.rank_d = base + cnt.rank;
    j.acc_count_d = base + cnt.accepted;
    j.nfill_d = c->placed_d + 2;
    MisArgs &ma = j.ma;
    ma.keys = pl.pre ? pl.pre->keys : c->keys; ma.seed = pl.pre ? sa.seedmap : nullptr; ma.seed_stamp = c->seed_stamp; ma.ncols = sa.ncols;
    ma.st = c->mis_st; ma.list = c->mis_list; ma.cnt = base + cnt.lists;
    ma.remaining = base + cnt.remaining; ma.acc_cnt = base + cnt.tile_accepted; ma.acc_cap = tile_cap;
    ma.acc_keys = c->mis_tile_keys; ma.info = j.info_d; ma.cut_dropped = j.info_d + 3;
    ma.nx = nx; ma.ny = ny; ma.R = R; ma.stage = 1; ma.bx = sa.bx; ma.by = sa.by; ma.step = sa.step;
    ma.sparse = mode == KLT_REPLACING_SOME && pl.prefilter ? 1 : 0;
    j.pa = na;                                          // placement: the accepted candidates never exclude each other
    j.pa.d = -1; j.pa.cell = 1; j.pa.cell_magic = 0u; j.pa.gw = j.pa.gh = 1; j.pa.grid_in_lds = 1; j.pa.grid_global = nullptr;
    j.pa.keys = c->keys2; j.pa.nkeys = (int)j.np2;
    j.sa = sa;
    consume.e = nullptr;                                // the job frees the score set when it is through with it
    if (int rc = select_job_start(c, j)) return rc;
    if (int rc = select_job_rounds(c, j)) return rc;
    c->sel_job = std::move(job);
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

// the greedy walk over sorted `keys`
int run_nms(klt_ctx *c, NmsArgs &na, const unsigned long long *keys, int nkeys, const QuotaArgs *qa, int ncols, int nrows)
{
    na.keys = keys;
    na.nkeys = nkeys;
    return enqueue_walk(c, na, qa, ncols, nrows);
}

// ---- sorted serial walk (KLT_OPT_SELECT_PARALLEL_NMS = 0, or an exclusion square too large for the LDS tile).  Leaves the
// selection enqueued in full (or, behind the prefilter, complete) and the sorted keys it walked in sorted_keys / sorted_count.
int serial_selection(klt_ctx *c, const SelPlan &pl, const SelectArgs &sa, NmsArgs &na, const QuotaArgs *qa)
{
    const int n = na.nfeat;
    if (qa) c->grid_path = 2;
    c->pick = klt_select_pick{0, 0, pl.prefilter ? 1 : 0, 1, 0, 0, 0, 0, na.grid_in_lds ? 0 : 1, 0};      // klt_select_pick_path
    const long long ncand = (long long)sa.nx * sa.ny, npow2 = sa.npow2;
    // top-K prefilter: sort only the candidates the greedy walk can plausibly reach (one small D2H read-back)
    if (pl.prefilter) {
        if (int rc = ensure(c, c->keys2, c->keys2_cap, (size_t)npow2)) return rc;
        size_t hcap = c->topk_hist ? 8192 + 4 : 0;
        if (int rc = ensure(c, c->topk_hist, hcap, (size_t)8192 + 4)) return rc;
        if (int rc = ensure(c, c->fl_snapshot, c->fl_snapshot_cap, (size_t)n)) return rc;
        HIPCHK(c, hipMemsetAsync(c->topk_hist, 0, (8192 + 4) * sizeof(unsigned), c->stream));
        unsigned info[4] = {0, 0, 0, 0};
        {
            TimerScope t(c, F_SORT, (double)ncand * 16);
            launch_topk_prefilter(c->stream, c->keys, (int)ncand, (unsigned)pl.target, c->topk_hist, c->topk_hist + 8192, c->keys2);
        }
        HIPCHK(c, hipMemcpyAsync(info, c->topk_hist + 8192, sizeof(info), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const long long kept = info[3], valid = info[2];
        const long long np2 = pow2_at_least_2048(kept);
        if (kept < np2) HIPCHK(c, hipMemsetAsync(c->keys2 + kept, 0, (size_t)(np2 - kept) * sizeof(unsigned long long), c->stream));
        { TimerScope t(c, F_SORT, (double)np2 * 16); launch_sort_desc(c->stream, c->keys2, (int)np2); }
        HIPCHK(c, hipMemcpyAsync(c->fl_snapshot, na.fl, (size_t)n * sizeof(klt_feat), hipMemcpyDefault, c->stream));
        if (int rc = run_nms(c, na, c->keys2, (int)kept, qa, sa.ncols, sa.nrows)) return rc;
        c->sorted_keys = c->keys2; c->sorted_count = (int)kept;
        int res[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(res, c->placed_d, sizeof(res), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!(res[1] && kept < valid)) { HIPCHK(c, hipGetLastError()); return KLT_OK; }
        // the kept candidates ran out before the list was full: restore the list and take the full sort
        if (int rc = restore_list(c, na.fl, n)) return rc;
        c->pick.attempts = 2;
    }
    { TimerScope t(c, F_SORT, (double)npow2 * 16); launch_sort_desc(c->stream, c->keys, (int)npow2); }
    if (int rc = run_nms(c, na, c->keys, (int)(ncand < npow2 ? ncand : npow2), qa, sa.ncols, sa.nrows)) return rc;
    c->sorted_keys = c->keys; c->sorted_count = (int)(ncand < npow2 ? ncand : npow2);
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}
}  // namespace

extern "C" {

// The half of a selection that depends on the pixels only -- summed-area tables and the eigenvalue of every candidate window
// (goodFeaturesUtils.pyx:17-73) -- for the level-0 images of `slot`, ahead of the selection itself: on the build stream when
// KLT_OPT_BUILD_STREAM is on, where it overlaps the tracker and the minimum-distance passes of the previous frame.
int klt_select_prepare_async(klt_ctx *c, int slot)
{
    if (int rc = check_ready(c)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    if (!s->pyr_valid) return fail(c, KLT_ERR_STATE, "klt_select_prepare_async: the slot's pyramids are not built");
    const int nc = s->nc, nr = s->nr;
    const size_t N = (size_t)nc * nr;
    SelGeom g;
    if (int rc = select_geometry(c, nc, nr, &g)) return rc;
    if (g.ncand <= 0) return KLT_OK;
    WorkScope work_scope{c};
    if (c->build_stream_on) {
        if (!c->bstream) HIPCHK(c, hipStreamCreateWithFlags(&c->bstream, hipStreamNonBlocking));
        if (!s->built_on_bstream) {             // built on the main stream: behind everything there
            hipEvent_t mark;
            if (int rc = fresh_event(c, &mark)) return rc;
            HIPCHK(c, hipEventRecord(mark, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->bstream, mark, 0));
        }
        // (the set being replaced was last read by a selection, and selections synchronise the main stream before they return)
        c->work = c->bstream;
    } else {
        if (int rc = wait_built(c, s)) return rc;
        for (auto &e : c->pre)                  // an earlier preparation on the build stream shares the table scratch
            if (e.ev && event_live(c, e.ev_serial)) HIPCHK(c, hipStreamWaitEvent(c->stream, e.ev, 0));
    }
    if (int rc = ensure_level0_records(c, s)) return rc;      // (a lean slot: made on the main stream, this one ordered behind it)
    // the set that already belongs to these contents, else a free one, else the oldest
    ScoreCache *e = nullptr;
    for (auto &x : c->pre) if (x.gen == s->gen) { e = &x; break; }
    if (!e) for (auto &x : c->pre) if (!x.gen) { e = &x; break; }
    if (!e) {
        const ScoreCache *busy = c->sel_job ? c->sel_job->pre : nullptr;      // (a pending selection still reads its set)
        for (auto &x : c->pre) if (&x != busy && (!e || x.stamp < e->stamp)) e = &x;
    }
    if (int rc = ensure(c, c->sat_pre, c->sat_pre_cap, 3 * N + KLT_SAT_PAD)) return rc;
    if (int rc = ensure(c, e->keys, e->cap, (size_t)g.npow2)) return rc;
    e->gen = 0;
    SelectArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.sat = c->sat_pre; sa.keys = e->keys;
    fill_select_geometry(sa, nc, nr, g, select_min_eig(c->p));
    // the tables' column pass and the eigenvalue keys in one launch where that applies (sat_pipeline.hip: the column-summed tables never
    // reach HBM); KLT_FUSED_COLS_EIGEN=0: the two separate kernels
    static const bool fused_cols_eigen = !(getenv("KLT_FUSED_COLS_EIGEN") && atoi(getenv("KLT_FUSED_COLS_EIGEN")) == 0);
    if (fused_cols_eigen && c->sat_variant == 1 && sat_cols_eigen_ok(sa)) {
        if (int rc = enqueue_sat(c, c->work, s->lv[0].gx, s->lv[0].gy, c->sat_pre, nc, nr, true)) return rc;
        int e2;
        { TimerScope t(c, F_EIGEN, 12.0 * N + (double)g.ncand * 8);
          e2 = launch_sat_cols_eigen_pipe(c->work, c->sat_pre, sa); }
        if (e2 > 0) return fail(c, KLT_ERR_DEVICE, std::string("column pass + eigenvalue keys: ") + hipGetErrorString((hipError_t)e2));
        if (e2 < 0) {
            // the fused kernel does not take this geometry after all: the column pass and the keys as two launches (no keys were written,
            // and the score set is only stamped below, after a launch that did write them)
            if (int rc = enqueue_sat_cols(c, c->work, c->sat_pre, nc, nr)) return rc;
            TimerScope t(c, F_EIGEN, 12.0 * N + (double)g.ncand * 8);
            launch_eigen_hist(c->work, sa);
        } else {
            c->score_cols_path = KLT_SCORE_FUSED_KEYS;
        }
    } else {
        if (int rc = enqueue_sat(c, c->work, s->lv[0].gx, s->lv[0].gy, c->sat_pre, nc, nr)) return rc;
        TimerScope t(c, F_EIGEN, 12.0 * N + (double)g.ncand * 8);
        launch_eigen_hist(c->work, sa);
    }
    if (int rc = fresh_event(c, &e->ev, &e->ev_serial)) return rc;
    HIPCHK(c, hipEventRecord(e->ev, c->work));
    e->gen = s->gen; e->stamp = ++c->pre_stamp;
    e->nc = nc; e->nr = nr; e->bx = g.bx; e->by = g.by; e->hw = g.hw; e->hh = g.hh; e->step = g.step; e->nx = g.nx; e->ny = g.ny;
    e->min_eig = sa.min_eig;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_select_begin_async(klt_ctx *c, int slot, int mode, int use_pyramid, int fb, int n)
{
    if (int rc = check_ready(c)) return rc;
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    if (mode != KLT_SELECTING_ALL && mode != KLT_REPLACING_SOME) return fail(c, KLT_ERR_ARG, "bad selection mode");
    if (n <= 0) return fail(c, KLT_ERR_ARG, "nFeatures must be positive");
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    const int nc = s->nc, nr = s->nr;
    FeatBuf *b;
    if (int rc = get_fb(c, fb, n, &b)) return rc;
    SelGeom geom;
    if (int rc = select_geometry(c, nc, nr, &geom)) return rc;
    if (int rc = check_select_mask(c, nc, nr)) return rc;

    if (int rc = ensure_select_scratch(c, (size_t)nc * nr, geom.npow2)) return rc;
    const float *img, *gx, *gy;
    if (int rc = select_planes(c, s, use_pyramid, &img, &gx, &gy)) return rc;
    c->last_sel[0] = img; c->last_sel[1] = gx; c->last_sel[2] = gy;
    c->sel_nc = nc; c->sel_nr = nr; c->sel_nx = geom.nx; c->sel_ny = geom.ny; c->sel_npow2 = (int)geom.npow2;

    const SelPlan plan = plan_selection(c, s, geom, mode, use_pyramid, n);
    c->sel_valmap = !plan.pre;
    Consume consume{plan.pre};
    if (plan.pre) {
        if (event_live(c, plan.pre->ev_serial)) HIPCHK(c, hipStreamWaitEvent(c->stream, plan.pre->ev, 0));
        else if (c->bstream && !c->capturing) HIPCHK(c, hipStreamSynchronize(c->bstream));
    } else {
        // summed-area tables (goodFeaturesUtils.pyx:49-51)
        if (int rc = enqueue_sat(c, c->stream, gx, gy, c->sat, nc, nr)) return rc;
    }
    const uint8_t *seed = nullptr;
    const bool live_squares = mode == KLT_REPLACING_SOME && plan.d >= 0;
    if (live_squares || c->mask) {
        if (int rc = begin_seed_map(c, nc, nr, &seed)) return rc;
        if (live_squares) fill_live_squares(c, b->d, n, nc, nr, plan.d);
        if (c->mask) fill_select_mask(c, nc, nr);
    }

    SelectArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.sat = c->sat; sa.valmap = c->valmap; sa.keys = c->keys; sa.seedmap = seed; sa.seed_stamp = c->seed_stamp;
    fill_select_geometry(sa, nc, nr, geom, plan.min_eig);
    if (c->score_override_n) {
        const int given = c->score_override_n;
        c->score_override_n = 0;
        if (given != geom.ncand) return fail(c, KLT_ERR_ARG, "score override does not match the candidate grid");
        sa.val_in = c->score_override;
    }
    if (!plan.parallel_nms) { TimerScope t(c, F_EIGEN, 12.0 * nc * nr + (double)geom.ncand * (4 + 8)); launch_eigen(c->stream, sa); }
    NmsArgs na;
    if (int rc = make_nms_args(c, b->d, n, mode == KLT_SELECTING_ALL, plan.d, nc, nr, na)) return rc;
    if (c->select_aff_state >= 0) {
        AffState &as = c->aff[c->select_aff_state];
        if (as.n < n) return fail(c, KLT_ERR_STATE, "affine state smaller than the feature list");
        na.aff_rec = as.rec;
    }
    QuotaArgs qa;
    const bool quota = c->sel_grid.cell_width > 0;                       // klt_set_select_grid
    if (quota)
        if (int rc = make_quota_args(c, nc, nr, qa)) return rc;
    if (plan.parallel_nms) return begin_parallel_selection(c, plan, sa, na, mode, consume, quota ? &qa : nullptr);
    return serial_selection(c, plan, sa, na, quota ? &qa : nullptr);
}

int klt_select_finish(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    if (!c->sel_job) return KLT_OK;                       // nothing pending (or a path that completes in klt_select_begin_async)
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<SelectJob> job = std::move(c->sel_job);
    return select_job_finish(c, *job);
}

int klt_select_async(klt_ctx *c, int slot, int mode, int use_pyramid, int fb, int n)
{
    if (int rc = klt_select_begin_async(c, slot, mode, use_pyramid, fb, n)) return rc;
    const int rc = klt_select_finish(c);
    return rc > 0 ? KLT_OK : rc;
}

int klt_select(klt_ctx *c, int slot, int mode, int use_pyramid, klt_feat *inout, int n, int *n_placed)
{
    if (!c || !inout) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = klt_featbuf_upload(c, kFbSyncOut, inout, n)) return rc;
    if (int rc = klt_select_async(c, slot, mode, use_pyramid, kFbSyncOut, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, inout, n)) return rc;
    if (n_placed) {
        HIPCHK(c, hipMemcpy(n_placed, c->placed_d, sizeof(int), hipMemcpyDeviceToHost));
    }
    return KLT_OK;
}

// _enforceMinimumDistance (selectGoodFeatures.py:45-135) as the reference's callers may use it on its own: the greedy walk over a
// GIVEN candidate list in the GIVEN order (keys as klt_download_sorted_candidates describes them: f32 bits of val << 32 | x << 16 | y;
// the caller has dropped the candidates the walk would skip without effect -- val below min_eigenvalue, positions inside the squares of
// live features when these are kept), filling the list's free slots: every slot in rank order when overwrite_all, the lost ones otherwise.
int klt_min_distance_walk(klt_ctx *c, const uint64_t *keys, int nkeys, int ncols, int nrows, int mindist, int overwrite_all,
                          klt_feat *inout, int n, int *n_placed)
{
    if (!c || !inout || (!keys && nkeys > 0)) return fail(c, KLT_ERR_ARG, "null argument");
    if (nkeys < 0 || n <= 0 || ncols <= 0 || nrows <= 0 || ncols > 65535 || nrows > 65535) return fail(c, KLT_ERR_ARG, "bad argument");
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    // every candidate inside the image (the reference asserts the same when the walk reaches the point, selectGoodFeatures.py:90-91): the
    // kernel marks accepted candidates in a grid of ncols x nrows cells and checks nothing, a position outside would be a write outside it
    for (int i = 0; i < nkeys; i++) {
        if (keys[i] == 0ull) return fail(c, KLT_ERR_ARG, "a zero key (value 0.0 at (0, 0)) is the walk's end mark, not a candidate");
        const int x = klt_key_x(keys[i]), y = klt_key_y(keys[i]);
        if (x >= ncols || y >= nrows) {
            char msg[128];
            snprintf(msg, sizeof msg, "candidate %d at (%d, %d) lies outside the %d x %d image", i, x, y, ncols, nrows);
            return fail(c, KLT_ERR_ARG, msg);
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int fb = kFbSyncOut;
    if (int rc = klt_featbuf_upload(c, fb, inout, n)) return rc;
    if (int rc = ensure(c, c->keys2, c->keys2_cap, (size_t)nkeys + 1)) return rc;
    if (nkeys) HIPCHK(c, hipMemcpyAsync(c->keys2, keys, (size_t)nkeys * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->keys2 + nkeys, 0, sizeof(uint64_t), c->stream));            // a zero key ends the walk
    NmsArgs na;
    const int d = (mindist < 0 ? 0 : mindist) - 1;        // :61 (and :241-243 for a negative minimum distance)
    if (int rc = make_nms_args(c, c->fbs[fb].d, n, overwrite_all != 0, d, ncols, nrows, na)) return rc;
    if (!na.grid_in_lds) HIPCHK(c, hipMemsetAsync(c->grid, 0, (size_t)na.gw * na.gh * sizeof(uint32_t), c->stream));
    na.keys = c->keys2; na.nkeys = nkeys + 1;
    if (const int e = launch_nms(c->stream, na, nullptr)) return fail(c, KLT_ERR_DEVICE, std::string("nms launch: ") + hipGetErrorString((hipError_t)e));
    c->sorted_keys = nullptr; c->sorted_count = 0;
    if (int rc = klt_featbuf_download(c, fb, inout, n)) return rc;
    if (n_placed) HIPCHK(c, hipMemcpy(n_placed, c->placed_d, sizeof(int), hipMemcpyDeviceToHost));
    return KLT_OK;
}

int klt_select_dims(klt_ctx *c, int what, int *ncols, int *nrows)
{
    if (!c || what < 0 || what > 3) return fail(c, KLT_ERR_ARG, "bad argument");
    if (c->sel_nc == 0) return fail(c, KLT_ERR_STATE, "no selection has run");
    if (ncols) *ncols = what == 3 ? c->sel_nx : c->sel_nc;
    if (nrows) *nrows = what == 3 ? c->sel_ny : c->sel_nr;
    return KLT_OK;
}

int klt_download_select_f32(klt_ctx *c, int what, float *dst)
{
    if (!c || !dst || what < 0 || what > 3) return fail(c, KLT_ERR_ARG, "bad argument");
    if (c->sel_nc == 0) return fail(c, KLT_ERR_STATE, "no selection has run");
    if (what == 3 && !c->sel_valmap) return fail(c, KLT_ERR_STATE, "the last selection used prepared scores: no eigenvalue map was written");
    const float *src = what == 3 ? c->valmap : c->last_sel[what];
    const size_t cnt = what == 3 ? (size_t)c->sel_nx * c->sel_ny : (size_t)c->sel_nc * c->sel_nr;
    HIPCHK(c, hipSetDevice(c->device));
    return download_plane(c, src, what == 3 ? 1 : KLT_PIX_STRIDE, cnt, dst);     // image, gradx, grady: planes of pixel records
}

int klt_download_prepared_keys(klt_ctx *c, int slot, uint64_t *dst, size_t capacity, int *nx, int *ny)
{
    if (int rc = check_ready(c)) return rc;
    if (!dst) return fail(c, KLT_ERR_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    SelGeom g;
    if (int rc = select_geometry(c, s->nc, s->nr, &g)) return rc;
    const ScoreCache *e = find_scores(c, s, g, select_min_eig(c->p));
    if (!e) return fail(c, KLT_ERR_STATE, "no prepared scores for the slot's contents under the current parameters (klt_select_prepare_async)");
    if (nx) *nx = e->nx;
    if (ny) *ny = e->ny;
    const size_t count = (size_t)e->nx * e->ny;
    if (capacity < count) return fail(c, KLT_ERR_ARG, "klt_download_prepared_keys: capacity smaller than nx * ny");
    // the set's own event where the ring still holds it, else whatever stream it may have been scored on
    if (event_live(c, e->ev_serial)) HIPCHK(c, hipEventSynchronize(e->ev));
    else { HIPCHK(c, hipStreamSynchronize(c->stream)); if (c->bstream) HIPCHK(c, hipStreamSynchronize(c->bstream)); }
    HIPCHK(c, hipMemcpy(dst, e->keys, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return KLT_OK;
}

int klt_select_score_path(klt_ctx *c, int *rows, int *cols)
{
    if (!c) return KLT_ERR_ARG;
    if (c->score_rows_path < 0 || c->score_cols_path < 0) return fail(c, KLT_ERR_STATE, "no summed-area tables have been built yet");
    if (rows) *rows = c->score_rows_path;
    if (cols) *cols = c->score_cols_path;
    return KLT_OK;
}

int klt_select_pick_path(klt_ctx *c, klt_select_pick *out)
{
    if (!c || !out) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    if (c->pick.walk < 0) return fail(c, KLT_ERR_STATE, "no selection has completed yet");
    *out = c->pick;
    return KLT_OK;
}

int klt_set_score_override(klt_ctx *c, const float *val, int count)
{
    if (!c || !val || count <= 0) return fail(c, KLT_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure(c, c->score_override, c->score_override_cap, (size_t)count)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->score_override, val, (size_t)count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->score_override_n = count;
    return KLT_OK;
}

int klt_set_select_grid(klt_ctx *c, const klt_select_grid *g)
{
    if (!c) return KLT_ERR_ARG;
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    if (!g || g->cell_width == 0) { c->sel_grid = klt_select_grid{0, 0, 0}; return KLT_OK; }
    if (g->cell_width < 1 || g->cell_height < 1) return fail(c, KLT_ERR_ARG, "selection grid: cell_width and cell_height must be at least 1");
    if (g->max_per_cell < 1 || g->max_per_cell > 65535) return fail(c, KLT_ERR_ARG, "selection grid: max_per_cell must lie in 1 .. 65535");
    c->sel_grid = *g;
    return KLT_OK;
}

int klt_select_grid_path(klt_ctx *c) { return c ? c->grid_path : KLT_ERR_ARG; }

// the context has no mask from here on (what a failed klt_set_select_mask* leaves as well)
static void drop_select_mask(klt_ctx *c) { c->mask = nullptr; c->mask_nc = c->mask_nr = 0; }

static int select_mask_args(klt_ctx *c, int ncols, int nrows)
{
    if (ncols <= 0 || nrows <= 0 || (long long)ncols * nrows > kMaxFramePixels) return fail(c, KLT_ERR_ARG, "bad selection mask size");
    return 0;
}

int klt_set_select_mask(klt_ctx *c, const uint8_t *mask, int ncols, int nrows, int pitch)
{
    if (!c) return KLT_ERR_ARG;
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    if (!mask) { drop_select_mask(c); return KLT_OK; }
    if (int rc = select_mask_args(c, ncols, nrows)) return rc;
    if (pitch < ncols) return fail(c, KLT_ERR_ARG, "selection mask: pitch smaller than ncols");
    HIPCHK(c, hipSetDevice(c->device));
    drop_select_mask(c);
    const size_t N = (size_t)ncols * nrows;
    if (int rc = ensure(c, c->mask_own, c->mask_own_cap, (N + 15) & ~(size_t)15)) return rc;
    // rows packed on the way (the plane is the library's: the kernel then reads a host mask and a device mask alike); behind whatever
    // still reads the plane's previous contents on the stream
    HIPCHK(c, hipMemcpy2DAsync(c->mask_own, (size_t)ncols, mask, (size_t)pitch, (size_t)ncols, (size_t)nrows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mask = c->mask_own; c->mask_nc = ncols; c->mask_nr = nrows;
    return KLT_OK;
}

int klt_set_select_mask_device(klt_ctx *c, const uint8_t *dev_mask, int ncols, int nrows)
{
    if (!c) return KLT_ERR_ARG;
    if (c->sel_job) return fail(c, KLT_ERR_STATE, "a selection is pending: klt_select_finish first");
    if (!dev_mask) { drop_select_mask(c); return KLT_OK; }
    if (int rc = select_mask_args(c, ncols, nrows)) return rc;
    if ((uintptr_t)dev_mask & 15) return fail(c, KLT_ERR_ARG, "selection mask: the device address must be a multiple of 16 (it is read 16 bytes at a time)");
    c->mask = dev_mask; c->mask_nc = ncols; c->mask_nr = nrows;
    return KLT_OK;
}

int klt_download_sorted_candidates(klt_ctx *c, float *val, int32_t *x, int32_t *y, int n, int *n_valid)
{
    if (!c || !val || !x || !y || n < 0) return fail(c, KLT_ERR_ARG, "bad argument");
    if (c->sel_nc == 0) return fail(c, KLT_ERR_STATE, "no selection has run");
    if (!c->sorted_keys) return fail(c, KLT_ERR_STATE, "the last selection kept no sorted candidate list (KLT_OPT_SELECT_PARALLEL_NMS = 0 keeps one)");
    if (n > c->sorted_count) n = c->sorted_count;
    std::vector<unsigned long long> h((size_t)(n > 0 ? n : 1));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(h.data(), c->sorted_keys, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int k = 0;
    for (; k < n && h[k] != 0ull; k++) {
        val[k] = klt_key_val(h[k]);
        x[k] = klt_key_x(h[k]);
        y[k] = klt_key_y(h[k]);
    }
    if (n_valid) *n_valid = k;
    return KLT_OK;
}

}  // extern "C"
