// api_track.hip -- the tracker (trackFeatures.py:205-409): single-pair and batched launches with their XCD-aware feature orders, the
// constant-velocity prediction, the iteration counters behind the roofline figures; and what every launch on a frame pair shares
// (klt_context.h lists it).  The kernels: track_kernels.hip, track_light_kernels.hip.
#include "klt_context.h"

// The caches of feature orders and descriptor tables: the entry that `match` accepts, or null ...
template <class Entry, class Match>
static Entry *cache_find(std::vector<Entry> &v, Match match)
{
    for (Entry &e : v)
        if (match(e)) return &e;
    return nullptr;
}

// ... and the place of a new entry: appended while the cache holds fewer than `capacity`, else the least recently used entry's (the
// first one with the smallest `used` stamp), whose contents the caller replaces
template <class Entry>
static Entry *cache_place(std::vector<Entry> &v, size_t capacity)
{
    if (v.size() < capacity) {
        v.emplace_back();
        return &v.back();
    }
    Entry *lru = &v[0];
    for (Entry &e : v)
        if (e.used < lru->used) lru = &e;
    return lru;
}

namespace kltapi {

int check_pair(klt_ctx *c, int slot1, int slot2, Slot **p1, Slot **p2, bool lazy_ok /* = false */)
{
    if (int rc = get_slot(c, slot1, p1, false)) return rc;
    if (int rc = get_slot(c, slot2, p2, false)) return rc;
    Slot *s1 = *p1, *s2 = *p2;
    if (!s1->pyr_valid || !s2->pyr_valid) return fail(c, KLT_ERR_STATE, "pyramids of both slots must be built before tracking");
    if (int rc = wait_built(c, s1)) return rc;
    if (int rc = wait_built(c, s2)) return rc;
    if (s1->nc != s2->nc || s1->nr != s2->nr || s1->nlev != s2->nlev || s1->ss != s2->ss)
        return fail(c, KLT_ERR_ARG, "the two frames differ in size");            // trackFeatures.py:156-159, :217
    if (!lazy_ok) {
        if (int rc = ensure_level0_records(c, s1)) return rc;
        if (int rc = ensure_level0_records(c, s2)) return rc;
    }
    return 0;
}

void level_planes(const Slot *s1, const Slot *s2, int l, const float *&i1, const float *&gx1, const float *&gy1, const float *&i2,
                  const float *&gx2, const float *&gy2)
{
    i1 = s1->lv[l].img; gx1 = s1->lv[l].gx; gy1 = s1->lv[l].gy;
    i2 = s2->lv[l].img; gx2 = s2->lv[l].gx; gy2 = s2->lv[l].gy;
}

// gain / bias tracking is offered by klt_track, klt_track_async and klt_track_batch_async alone: every other tracker entry point is refused
// while it is switched on, before anything is enqueued
int refuse_with_light(klt_ctx *c, const char *what)
{
    if (!c || !c->lightp.mode) return 0;
    return fail(c, KLT_ERR_STATE, std::string(what) + " is not offered together with lighting compensation (klt_set_light_params mode 1)");
}

int count_live(const klt_feat *f, int n)
{
    int k = 0;
    for (int i = 0; i < n; i++) k += f[i].val >= 0;
    return k;
}

int batch_arguments(klt_ctx *c, std::initializer_list<const int *> columns, int npairs, int n)
{
    const bool null_column = std::count(columns.begin(), columns.end(), nullptr) > 0;
    return null_column || npairs <= 0 || npairs > 65535 || n < 0 ? fail(c, KLT_ERR_ARG, "bad argument") : 0;
}

int batch_pair(klt_ctx *c, int slot1, int slot2, bool same_levels, std::vector<Slot *> &used, bool lazy_ok /* = false */)
{
    Slot *s1, *s2;
    if (int rc = check_pair(c, slot1, slot2, &s1, &s2, lazy_ok)) return rc;
    used.push_back(s1);
    used.push_back(s2);
    const Slot *first = used[0];
    if (s1->nc != first->nc || s1->nr != first->nr || (same_levels && s1->nlev != first->nlev))
        return fail(c, KLT_ERR_ARG, "all pairs of a batch must have the same frame size");
    return 0;
}

}  // namespace kltapi

int g_track_variant = getenv("KLT_TRACK_VARIANT") ? atoi(getenv("KLT_TRACK_VARIANT")) : 4;      // KLT_OPT_TRACK_VARIANT: read by launch_pairs and nowhere else

extern "C" {

static void fill_track_params(const klt_ctx *c, const Slot *s1, TrackArgs &a, int n)
{
    const klt_params &p = c->p;
    a.half_window = p.window_width / 2.0;
    a.borderx = p.borderx; a.bordery = p.bordery;
    a.n = n; a.nlevels = s1->nlev; a.window = p.window_width; a.max_iterations = p.max_iterations;
    a.use_max_residue = p.use_max_residue; a.retain = p.retainTrackers; a.ncols = s1->nc; a.nrows = s1->nr;
    a.small = p.min_determinant; a.th = p.min_displacement; a.step = p.step_factor; a.max_residue = p.max_residue;
    a.ss = (float)s1->ss;
    a.inv_ss = 1.0f / (float)s1->ss;
    a.tree_sums = c->track_tree_sums ? 1 : 0;
}

// the forward-backward launch on top (klt_track_fb*): the squared threshold as the kernels compare it
static void fill_fb_params(const klt_ctx *c, TrackArgs &a)
{
    a.fb = 1;
    a.fb_max_e2 = (double)c->fbp.max_error * (double)c->fbp.max_error;
}

// XCD-aware feature order (KLT_OPT_TRACK_XCD_ORDER): one permutation of 0..n-1 per pair of the launch.  It is only a locality
// hint (any permutation tracks every feature exactly once), so it is recomputed when the shape of the launch changes and every
// 64th launch (a sequence's features drift, and its lists alternate between two buffers); in between the stored one is reused.
// The orders are kept per set of INPUT lists (at most kBatchOrders sets, least recently used one replaced): a caller that rotates
// through many resident pairs -- each with its own list -- finds every list's own order again instead of tracking pair B in the
// order of pair A's rows.  A single-pair launch on a list seen for the FIRST time takes the context's shared order instead (refreshed every
// 64 launches): the rows of a sequence's feature table are all new buffers holding nearly the same
// positions, and an order kernel per frame would buy nothing; the second launch on the same buffer gives it its own entry.
static int set_track_order(klt_ctx *c, TrackArgs &a, int n, int chunk, const std::vector<const klt_feat *> &ins)
{
    const int npairs = (int)ins.size();
    klt_ctx::BatchOrder *bo = cache_find(c->batch_orders, [&](const klt_ctx::BatchOrder &e) { return e.in == ins; });
    if (npairs == 1) {
        bool seen = false;
        for (const klt_feat *p : c->seen_once) seen = seen || p == ins[0];
        if (!bo && !seen) {
            if (c->seen_once.size() >= 256) c->seen_once.erase(c->seen_once.begin());
            c->seen_once.push_back(ins[0]);
            bo = &c->shared_order;
        }
    }
    if (!bo) {
        bo = cache_place(c->batch_orders, klt_ctx::kBatchOrders);
        bo->in = ins;
        bo->n = -1;
    }
    bo->used = ++c->batch_clock;
    const size_t cap_before = bo->cap;
    if (int rc = ensure(c, bo->order, bo->cap, (size_t)n * npairs)) return rc;
    if (bo->cap != cap_before) bo->n = -1;               // a new buffer holds no order yet
    a.order = bo->order;
    a.order_chunk = chunk;
    a.order_refresh = (bo->n != n || bo->age >= 64) ? 1 : 0;
    if (a.order_refresh) { bo->n = n; bo->age = 0; }
    bo->age++;
    return 0;
}

// lazy: level 0 is the two slots' compact images (TrackLazyArgs; the kernels do not look at that level's gradient pointers)
static void fill_levels(const Slot *s1, const Slot *s2, TrackLevel *lv, bool lazy)
{
    for (int l = 0; l < s1->nlev; l++) {
        level_planes(s1, s2, l, lv[l].i1, lv[l].gx1, lv[l].gy1, lv[l].i2, lv[l].gx2, lv[l].gy2);
        lv[l].nc = s1->lv[l].nc; lv[l].nr = s1->lv[l].nr;
    }
    if (lazy) {
        lv[0].i1 = s1->l0img; lv[0].i2 = s2->l0img;
        lv[0].gx1 = lv[0].gy1 = lv[0].gx2 = lv[0].gy2 = nullptr;
    }
}

// what a forward-backward launch asks of a pair's three feature buffers (fb_back: a buffer or -1)
static int check_fb_buffers(klt_ctx *c, int fb_in, int fb_out, int fb_back)
{
    if (fb_in == fb_out || (fb_back >= 0 && (fb_back == fb_in || fb_back == fb_out)))
        return fail(c, KLT_ERR_ARG, "the forward-backward check needs fb_in, fb_out and fb_back pairwise distinct");
    if (fb_back < -1) return fail(c, KLT_ERR_ARG, "fb_back must be a feature buffer or -1");
    return 0;
}

// what a launch with a motion prior asks of a pair's guess list (klt_track_guess*): a feature buffer of its own next to the ones the
// launch writes (own_index; fb_back: a buffer or -1).  (It may be fb_in: every feature's guess is then its own position.)
static const char *const kGuessNotDistinct = "fb_guess must be distinct from fb_out and fb_back";
static int check_guess_buffer(klt_ctx *c, int fb_guess, int fb_out, int fb_back)
{
    return own_index(c, fb_guess, {fb_out, fb_back}, "fb_guess must be a feature buffer", kGuessNotDistinct);
}

// ... once the launch's own buffers exist: the guess list holds n records and shares no memory with them (own_records)
static int guess_records(klt_ctx *c, int fb_guess, int fb_out, int fb_back, int n, const klt_feat **guess)
{
    if (!fb_holds_records(c, fb_guess, n)) return fail(c, KLT_ERR_ARG, "the guess feature buffer holds fewer records than the feature list");
    *guess = c->fbs[fb_guess].d;
    return own_records(c, fb_guess, {fb_out, fb_back}, kGuessNotDistinct);
}

// A batched launch's descriptor table on the device.  It is uploaded only when none of the tables kept there holds it (found by hash; at
// most 256 tables, the least recently used one is replaced).  Pageable source: the runtime stages it before returning; stream order
// protects the launch that read the replaced table
static int upload_pair_table(klt_ctx *c, const std::vector<TrackPairDesc> &table, const TrackPairDesc **dev)
{
    const size_t bytes = table.size() * sizeof(TrackPairDesc);
    uint64_t hash = 1469598103934665603ull;
    const unsigned char *raw = reinterpret_cast<const unsigned char *>(table.data());
    for (size_t i = 0; i < bytes; i++) hash = (hash ^ raw[i]) * 1099511628211ull;
    klt_ctx::BatchTable *bt = cache_find(c->batch_tables, [&](const klt_ctx::BatchTable &e) {
        return e.hash == hash && e.host.size() == table.size() && std::memcmp(e.host.data(), table.data(), bytes) == 0;
    });
    if (!bt) {
        bt = cache_place(c->batch_tables, klt_ctx::kBatchTables);
        if (int rc = ensure(c, bt->dev, bt->cap, table.size())) return rc;
        HIPCHK(c, hipMemcpyAsync(bt->dev, table.data(), bytes, hipMemcpyHostToDevice, c->stream));
        bt->host = table;
        bt->hash = hash;
    }
    bt->used = ++c->batch_clock;
    *dev = bt->dev;
    return 0;
}

// The back half of every tracker entry point, from the launch's parameters to the marks on its slots: one request, one plan (plan_track,
// track_plan.h), and every step reads off the plan.  slots: those of the pairs, two each, built and of one size (check_pair).  table: a
// batched launch's descriptors with their lists filled in, or null for a single pair, whose lists are in `a`.
static int launch_pairs(klt_ctx *c, TrackGuessArgs &a, Slot *const *slots, int npairs, int n, bool fb, bool guess, std::vector<TrackPairDesc> *table)
{
    const int nslots = 2 * npairs, nlev = slots[0]->nlev;
    fill_track_params(c, slots[0], a, n);
    TrackRequest q = {};
    q.window = a.window; q.n = n; q.batched = table != nullptr; q.npairs = npairs;
    q.fb = fb; q.guess = guess; q.light = c->lightp.mode != 0; q.tree_sums = c->track_tree_sums; q.variant = g_track_variant;
    q.order = c->track_xcd_order && n >= 64 && !q.light; q.order_chunk = (n + 7) / 8;
    q.grad7 = merged_grad_ok(c); q.lazy_form = c->track_lazy_form;
    q.all_compact = true;
    for (int i = 0; i < nslots; i++) q.all_compact = q.all_compact && slots[i]->l0img_valid;
    const TrackPlan plan = plan_track(q);
    if (plan.refusal) return fail(c, KLT_ERR_ARG, plan.refusal);
    // KLT_OPT_L0_LAZY_GRAD: the slots without level-0 records get them here (one launch per KLT_MAX_BATCH slots); the fallback of a
    // launch that has a lazy form is not held against the slots
    if (plan.need_records)
        if (int rc = ensure_level0_records(c, slots, nslots, !plan.lazy_capable)) return rc;
    if (table) {
        for (int i = 0; i < npairs; i++) fill_levels(slots[2 * i], slots[2 * i + 1], (*table)[i].lv, plan.lazy);
        if (int rc = upload_pair_table(c, *table, &a.pairs)) return rc;
        a.npairs = npairs;
    } else {
        fill_levels(slots[0], slots[1], a.lv, plan.lazy);
    }
    if (fb) fill_fb_params(c, a);
    if (plan.uses_order) {
        // one permutation per pair, kept with the set of input lists (see set_track_order)
        std::vector<const klt_feat *> ins((size_t)npairs);
        for (int i = 0; i < npairs; i++) ins[i] = table ? (*table)[i].in : a.in;
        if (int rc = set_track_order(c, a, n, q.order_chunk, ins)) return rc;
    }
    {
        const double foot = 12.0 * (c->p.window_width + 1) * (c->p.window_width + 1);
        // (a lazy level 0 reads the 14 x 14 image patch around a footprint, 4 bytes per pixel, instead of the footprint's records)
        const double foot0 = plan.lazy ? 4.0 * 14 * 14 : foot;
        TimerScope t(c, F_TRACK, (double)npairs * n * (foot * 2 * (nlev - 1) + foot0 * 2 + 32), c->stream);   // refined by the caller from klt_track_stats
        launch_track(c->stream, plan, a, c->gauss[2].k, c->deriv[2].k);
    }
    if (plan.light_path) c->light_path = plan.light_path;
    // a launch that has a lazy form leaves its mark on the slots it read (their next build may be lean)
    for (int i = 0; i < nslots && plan.lazy_capable; i++) slots[i]->lazy_read = true;
    if (c->collect_stats)
        for (int i = 0; i < npairs; i++)
            launch_track_stats(c->stream, table ? (*table)[i].in : a.in, table ? (*table)[i].out : a.out, n, nlev, c->stats_d);
    if (int rc = mark_read(c, slots, nslots)) return rc;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

// klt_track_async (fb == false) and klt_track_fb_async (fb == true; fb_back = the buffer of the backward records or -1); guess == true:
// klt_track_guess_async and klt_track_fb_guess_async, with the predicted positions in fb_guess
static int track_single(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_out, int n, bool fb, int fb_back, bool guess = false,
                        int fb_guess = -1)
{
    if (int rc = check_ready(c)) return rc;
    if (fb || guess)
        if (int rc = refuse_with_light(c, fb ? "the forward-backward check" : "a motion prior")) return rc;
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (fb)
        if (int rc = check_fb_buffers(c, fb_in, fb_out, fb_back)) return rc;
    if (guess)
        if (int rc = check_guess_buffer(c, fb_guess, fb_out, fb ? fb_back : -1)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot *both[2];
    // (a launch that may have a lazy form looks after level 0 itself, launch_pairs; any other gets its records here, slot by slot)
    if (int rc = check_pair(c, slot1, slot2, &both[0], &both[1], track_lazy_rule(fb, guess, c->lightp.mode != 0))) return rc;
    if (int rc = lists_set(c, {fb_in}, n, false)) return rc;
    FeatBuf *bo;
    if (fb && fb_back >= 0)                                  // (may grow c->fbs: before any pointer into it is taken)
        if (int rc = get_fb(c, fb_back, n > 0 ? n : 1, &bo)) return rc;
    if (int rc = get_fb(c, fb_out, n > 0 ? n : 1, &bo)) return rc;
    TrackGuessArgs a;
    std::memset(&a, 0, sizeof(a));
    if (guess)
        if (int rc = guess_records(c, fb_guess, fb_out, fb ? fb_back : -1, n, &a.guess)) return rc;
    a.in = c->fbs[fb_in].d; a.out = bo->d;
    if (fb && fb_back >= 0) a.back = c->fbs[fb_back].d;
    return launch_pairs(c, a, both, 1, n, fb, guess, nullptr);
}

int klt_track_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_out, int n)
{
    return track_single(c, slot1, slot2, fb_in, fb_out, n, false, -1);
}

int klt_track_fb_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_out, int n, int fb_back)
{
    return track_single(c, slot1, slot2, fb_in, fb_out, n, true, fb_back);
}

int klt_track_guess_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_guess, int fb_out, int n)
{
    return track_single(c, slot1, slot2, fb_in, fb_out, n, false, -1, true, fb_guess);
}

int klt_track_fb_guess_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_guess, int fb_out, int n, int fb_back)
{
    return track_single(c, slot1, slot2, fb_in, fb_out, n, true, fb_back, true, fb_guess);
}

// constant-velocity prediction from the lists of the last two frames (predict_cv_kernel has the rule)
int klt_predict_cv_async(klt_ctx *c, int fb_prev, int fb_cur, int fb_guess, int n)
{
    if (int rc = check_ready(c)) return rc;
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (fb_guess == fb_prev || fb_guess == fb_cur) return fail(c, KLT_ERR_ARG, "fb_guess must be distinct from fb_prev and fb_cur");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = lists_set(c, {fb_prev, fb_cur}, n)) return rc;
    FeatBuf *bg;                                             // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_guess, n > 0 ? n : 1, &bg)) return rc;
    if (bg->d == c->fbs[fb_prev].d || bg->d == c->fbs[fb_cur].d)
        return fail(c, KLT_ERR_ARG, "fb_guess must be distinct from fb_prev and fb_cur");
    launch_predict_cv(c->stream, c->fbs[fb_prev].d, c->fbs[fb_cur].d, bg->d, n);
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_set_light_params(klt_ctx *c, const klt_light_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 0 && p->mode != 1) return fail(c, KLT_ERR_ARG, "lighting compensation mode must be 0 (off) or 1 (gain + bias)");
    c->lightp = *p;
    return KLT_OK;
}

int klt_track_light_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->light_path;
}

int klt_set_fb_params(klt_ctx *c, const klt_fb_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (!(p->max_error >= 0.f)) return fail(c, KLT_ERR_ARG, "fb max_error must be a number >= 0");      // (NaN fails the comparison)
    c->fbp = *p;
    return KLT_OK;
}

// klt_track_batch_async (fb == false) and klt_track_fb_batch_async (fb == true; fb_back may be null); fb_guess != null:
// klt_track_guess_batch_async, an entry of -1 = that pair has no guess list
static int track_batch(klt_ctx *c, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out, const int *fb_back, int npairs,
                       int n, bool fb, const int *fb_guess = nullptr)
{
    if (int rc = check_ready(c)) return rc;
    if (fb || fb_guess)
        if (int rc = refuse_with_light(c, fb ? "the forward-backward check" : "a motion prior")) return rc;
    if (int rc = batch_arguments(c, {slot1, slot2, fb_in, fb_out}, npairs, n)) return rc;
    if (fb_guess)
        for (int i = 0; i < npairs; i++) {
            if (fb_guess[i] == -1) continue;
            // (a guess list that another pair of the launch writes would be read while it changes: distinct from every pair's output)
            for (int j = 0; j < npairs; j++)
                if (int rc = check_guess_buffer(c, fb_guess[i], fb_out[j], -1)) return rc;
        }
    if (fb)
        for (int i = 0; i < npairs; i++)
            if (int rc = check_fb_buffers(c, fb_in[i], fb_out[i], fb_back ? fb_back[i] : -1)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<TrackPairDesc> table((size_t)npairs);
    std::vector<Slot *> used;
    for (int i = 0; i < npairs; i++) {
        FeatBuf *bo;                      // may grow c->fbs: do it before taking pointers into it
        if (int rc = get_fb(c, fb_out[i], n > 0 ? n : 1, &bo)) return rc;
        if (fb && fb_back && fb_back[i] >= 0)
            if (int rc = get_fb(c, fb_back[i], n > 0 ? n : 1, &bo)) return rc;
    }
    for (int i = 0; i < npairs; i++) {
        if (int rc = batch_pair(c, slot1[i], slot2[i], true, used, true)) return rc;
        if (int rc = lists_set(c, {fb_in[i]}, n, false)) return rc;
        std::memset(&table[i], 0, sizeof(TrackPairDesc));
        table[i].in = c->fbs[fb_in[i]].d;
        table[i].out = c->fbs[fb_out[i]].d;
        if (fb && fb_back && fb_back[i] >= 0) table[i].back = c->fbs[fb_back[i]].d;
        if (fb_guess && fb_guess[i] >= 0)
            for (int j = 0; j < npairs; j++)                 // (next to this pair's output and every other pair's)
                if (int rc = guess_records(c, fb_guess[i], fb_out[i], fb_out[j], n, &table[i].guess)) return rc;
    }
    TrackGuessArgs a;
    std::memset(&a, 0, sizeof(a));
    return launch_pairs(c, a, used.data(), npairs, n, fb, fb_guess != nullptr, &table);
}

int klt_track_batch_async(klt_ctx *c, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out, int npairs, int n)
{
    return track_batch(c, slot1, slot2, fb_in, fb_out, nullptr, npairs, n, false);
}

int klt_track_fb_batch_async(klt_ctx *c, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out, const int *fb_back,
                             int npairs, int n)
{
    return track_batch(c, slot1, slot2, fb_in, fb_out, fb_back, npairs, n, true);
}

int klt_track_guess_batch_async(klt_ctx *c, const int *slot1, const int *slot2, const int *fb_in, const int *fb_guess, const int *fb_out,
                                int npairs, int n)
{
    if (!fb_guess) return fail(c, KLT_ERR_ARG, "bad argument");
    return track_batch(c, slot1, slot2, fb_in, fb_out, nullptr, npairs, n, false, fb_guess);
}

int klt_track_guess(klt_ctx *c, int slot1, int slot2, klt_feat *inout, const klt_feat *guess, int n, int *n_tracked)
{
    if (!c || !inout || !guess) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = refuse_with_light(c, "a motion prior")) return rc;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, inout, n)) return rc;      // (the download below synchronises: both lists are ours until then)
    if (int rc = klt_featbuf_upload_async(c, kFbSyncGuess, guess, n)) return rc;
    if (int rc = klt_track_guess_async(c, slot1, slot2, kFbSyncIn, kFbSyncGuess, kFbSyncOut, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, inout, n)) return rc;
    if (n_tracked) *n_tracked = count_live(inout, n);
    return KLT_OK;
}

int klt_track(klt_ctx *c, int slot1, int slot2, klt_feat *inout, int n, int *n_tracked)
{
    if (!c || !inout) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, inout, n)) return rc;      // (the download below synchronises: `inout` is ours until then)
    if (int rc = klt_track_async(c, slot1, slot2, kFbSyncIn, kFbSyncOut, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, inout, n)) return rc;
    if (n_tracked) *n_tracked = count_live(inout, n);
    return KLT_OK;
}

int klt_track_fb(klt_ctx *c, int slot1, int slot2, klt_feat *inout, klt_feat *back, int n, int *n_tracked)
{
    if (!c || !inout) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = refuse_with_light(c, "the forward-backward check")) return rc;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, inout, n)) return rc;
    if (int rc = klt_track_fb_async(c, slot1, slot2, kFbSyncIn, kFbSyncOut, n, back ? kFbSyncBack : -1)) return rc;
    if (back)
        if (int rc = klt_featbuf_download(c, kFbSyncBack, back, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, inout, n)) return rc;
    if (n_tracked) *n_tracked = count_live(inout, n);
    return KLT_OK;
}

int klt_track_stats_reset(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    HIPCHK(c, hipMemsetAsync(c->stats_d, 0, (1 + 2 * KLT_MAX_LEVELS) * sizeof(unsigned long long), c->stream));
    c->collect_stats = true;
    return KLT_OK;
}

int klt_track_stats_read(klt_ctx *c, klt_track_stats *out)
{
    if (!c || !out) return fail(c, KLT_ERR_ARG, "null argument");
    unsigned long long h[1 + 2 * KLT_MAX_LEVELS];
    HIPCHK(c, hipMemcpyAsync(h, c->stats_d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->collect_stats = false;
    out->features = h[0];
    for (int l = 0; l < KLT_MAX_LEVELS; l++) { out->level_visits[l] = h[1 + l]; out->iterations[l] = h[1 + KLT_MAX_LEVELS + l]; }
    return KLT_OK;
}

}  // extern "C"
