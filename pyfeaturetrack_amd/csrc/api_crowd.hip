// api_crowd.hip -- the crowding check (not in the reference): parameters, the single-list, batched and synchronous
// entry points.  The rule stands in include/klt_gpu.h, the kernels in crowd_kernels.hip.
#include "klt_context.h"

static const char *const kCrowdOff = "the crowding check is off (klt_set_crowd_params mode 0)";
static const char *const kCrowdNoBuffer = "fb_crowd must be a feature buffer";
static const char *const kCrowdNotDistinct = "fb_crowd must be distinct from fb_out and fb_prev";
static const char *const kCrowdBatchNotDistinct = "every fb_crowd must be distinct from every other buffer of the batch";
static const char *const kCrowdOutShared = "two lists of the batch share fb_out";

// the cell grid of a frame: squares of max(r + 1, 16) pixels, doubled until there are at most 65536 of them (32400 at 4K with side 16)
static void fill_crowd_grid(const klt_crowd_params &p, CrowdArgs &a)
{
    a.ncols = p.ncols; a.nrows = p.nrows; a.r = p.min_distance - 1;
    long long side = p.min_distance > 16 ? p.min_distance : 16;
    for (;;) {
        a.gx = (int)((p.ncols + side - 1) / side); a.gy = (int)((p.nrows + side - 1) / side);
        if ((long long)a.gx * a.gy <= 65536) break;
        side *= 2;
    }
    a.side = (int)side;
}

// a list's slice of the scratch: the classified records and the grouped candidates (16 bytes each), the cells' counts and offsets, the
// states of a list too long for LDS, the round count; a multiple of 256 bytes
static size_t crowd_slice_bytes(int n, int ncells)
{
    const size_t b = (size_t)n * 32 + ((size_t)ncells * 2 + 1) * 4 + (n > kCrowdLdsStates ? (size_t)n * 4 : 0) + 16;
    return (b + 255) & ~(size_t)255;
}

static void fill_crowd_pair(klt_ctx *c, int i, int n, int ncells, int fb_out, int fb_prev, int fb_crowd, CrowdPair &p)
{
    std::memset(&p, 0, sizeof(p));
    p.out = c->fbs[fb_out].d;
    p.prev = fb_prev >= 0 ? reinterpret_cast<const klt_crowd *>(c->fbs[fb_prev].d) : nullptr;
    p.crowd = reinterpret_cast<klt_crowd *>(c->fbs[fb_crowd].d);
    unsigned char *base = c->crowd_scratch + (size_t)i * crowd_slice_bytes(n, ncells);
    p.info = reinterpret_cast<CrowdCand *>(base);
    p.sorted = reinterpret_cast<CrowdCand *>(base + (size_t)n * 16);
    p.cells = reinterpret_cast<int *>(base + (size_t)n * 32);
    p.starts = p.cells + ncells;
    p.state = p.starts + ncells + 1;
    p.rounds = p.state + (n > kCrowdLdsStates ? n : 0);
}

// the three launches: the two over the records are timed as one family, the resolve launch as another (klt_timing_enable:
// crowd_prepare + crowd_check is the check's cost)
static int enqueue_crowd(klt_ctx *c, const CrowdArgs &a, int nlists)
{
    const double list = (double)nlists * a.n * 16;
    { TimerScope t(c, F_CROWD_PREPARE, list * 3, c->stream); launch_crowd_prepare(c->stream, a); }
    { TimerScope t(c, F_CROWD_PREPARE, list * 0.5, c->stream); launch_crowd_rank(c->stream, a); }
    { TimerScope t(c, F_CROWD, list * 4, c->stream); launch_crowd_resolve(c->stream, a); }
    return 0;
}

extern "C" {

int klt_set_crowd_params(klt_ctx *c, const klt_crowd_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 0 && p->mode != 1) return fail(c, KLT_ERR_ARG, "crowding mode must be 0 (off) or 1 (on)");
    if (p->min_distance < 1) return fail(c, KLT_ERR_ARG, "crowding check: min_distance must be at least 1");
    if (p->mode == 1 && (p->ncols < 1 || p->ncols > 65535 || p->nrows < 1 || p->nrows > 65535))
        return fail(c, KLT_ERR_ARG, "crowding check: ncols and nrows must lie in 1 .. 65535");
    c->crowdp = *p;
    return KLT_OK;
}

int klt_crowd_check_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->crowd_path;
}

int klt_crowd_check_rounds(klt_ctx *c, int *rounds, int *phase_ticks)
{
    if (!c || !rounds) return fail(c, KLT_ERR_ARG, "null argument");
    if (!c->crowd_path || !c->crowd_rounds) return fail(c, KLT_ERR_STATE, "no crowding check has been launched");
    HIPCHK(c, hipSetDevice(c->device));
    int got[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(got, c->crowd_rounds, sizeof(got), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *rounds = got[0];
    if (phase_ticks)
        for (int i = 0; i < 3; i++) phase_ticks[i] = got[1 + i];
    return KLT_OK;
}

int klt_crowd_check_async(klt_ctx *c, int fb_out, int fb_prev, int fb_crowd, int n)
{
    if (!c) return KLT_ERR_ARG;
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (fb_prev < -1) return fail(c, KLT_ERR_ARG, "fb_prev must be a feature buffer or -1");
    if (int rc = own_index(c, fb_crowd, {fb_out, fb_prev}, kCrowdNoBuffer, kCrowdNotDistinct)) return rc;
    if (c->crowdp.mode == 0) return fail(c, KLT_ERR_STATE, kCrowdOff);
    if (n == 0) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = lists_set(c, {fb_out}, n)) return rc;
    if (fb_prev >= 0)
        if (int rc = lists_set(c, {fb_prev}, n)) return rc;
    if (int rc = own_records(c, fb_crowd, {fb_out, fb_prev}, kCrowdNotDistinct)) return rc;
    CrowdArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_crowd_grid(c->crowdp, a);
    a.n = n;
    if (int rc = ensure(c, c->crowd_scratch, c->crowd_scratch_cap, crowd_slice_bytes(n, a.gx * a.gy))) return rc;
    FeatBuf *bc;                                             // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_crowd, n, &bc)) return rc;
    fill_crowd_pair(c, 0, n, a.gx * a.gy, fb_out, fb_prev, fb_crowd, a.one);
    if (int rc = enqueue_crowd(c, a, 1)) return rc;
    c->crowd_path = 1;
    c->crowd_rounds = a.one.rounds;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_crowd_check_batch_async(klt_ctx *c, const int *fb_out, const int *fb_prev, const int *fb_crowd, int npairs, int n)
{
    if (!c) return KLT_ERR_ARG;
    if (!fb_out || !fb_crowd || npairs <= 0 || npairs > 65535 || n < 0) return fail(c, KLT_ERR_ARG, "bad argument");
    auto prev_of = [&](int i) { return fb_prev ? fb_prev[i] : -1; };
    // crowd records that another list of the launch reads or writes, a list that two of them rewrite: by index first ...
    for (int i = 0; i < npairs; i++) {
        if (prev_of(i) < -1) return fail(c, KLT_ERR_ARG, "fb_prev must be a feature buffer or -1");
        for (int j = 0; j < npairs; j++) {
            if (int rc = own_index(c, fb_crowd[i], {fb_out[j], prev_of(j), i != j ? fb_crowd[j] : -1}, kCrowdNoBuffer, kCrowdBatchNotDistinct))
                return rc;
            if (i != j && fb_out[i] == fb_out[j]) return fail(c, KLT_ERR_ARG, kCrowdOutShared);
        }
    }
    if (c->crowdp.mode == 0) return fail(c, KLT_ERR_STATE, kCrowdOff);
    if (n == 0) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < npairs; i++) {
        if (int rc = lists_set(c, {fb_out[i]}, n)) return rc;
        if (prev_of(i) >= 0)
            if (int rc = lists_set(c, {prev_of(i)}, n)) return rc;
    }
    // ... then by address
    for (int i = 0; i < npairs; i++)
        for (int j = 0; j < npairs; j++) {
            if (int rc = own_records(c, fb_crowd[i], {fb_out[j], prev_of(j), i != j ? fb_crowd[j] : -1}, kCrowdBatchNotDistinct)) return rc;
            if (i != j && c->fbs[fb_out[i]].d == c->fbs[fb_out[j]].d) return fail(c, KLT_ERR_ARG, kCrowdOutShared);
        }
    CrowdArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_crowd_grid(c->crowdp, a);
    a.n = n;
    const int ncells = a.gx * a.gy;
    if (int rc = ensure(c, c->crowd_scratch, c->crowd_scratch_cap, (size_t)npairs * crowd_slice_bytes(n, ncells))) return rc;
    for (int i = 0; i < npairs; i++) {
        FeatBuf *bc;                                         // may grow c->fbs: do it before taking pointers into it
        if (int rc = get_fb(c, fb_crowd[i], n, &bc)) return rc;
    }
    std::vector<CrowdPair> table((size_t)npairs);
    for (int i = 0; i < npairs; i++) fill_crowd_pair(c, i, n, ncells, fb_out[i], prev_of(i), fb_crowd[i], table[i]);
    if (int rc = send_if_changed(c, c->crowd_table, table, &a.pairs)) return rc;
    a.npairs = npairs;
    if (int rc = enqueue_crowd(c, a, npairs)) return rc;
    c->crowd_path = 2;
    c->crowd_rounds = table[0].rounds;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_crowd_check(klt_ctx *c, klt_feat *out, const klt_crowd *prev, klt_crowd *crowd, int n, int *n_crowded)
{
    if (!c || !out || !crowd) return fail(c, KLT_ERR_ARG, "null argument");
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (c->crowdp.mode == 0) return fail(c, KLT_ERR_STATE, kCrowdOff);
    if (n_crowded) *n_crowded = 0;
    if (n == 0) return KLT_OK;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, out, n)) return rc;      // (the downloads below synchronise: the arrays are ours until then)
    if (prev)
        if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, reinterpret_cast<const klt_feat *>(prev), n)) return rc;
    if (int rc = klt_crowd_check_async(c, kFbSyncOut, prev ? kFbSyncIn : -1, kFbSyncOwn, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(crowd), n)) return rc;
    if (n_crowded) {
        int count = 0;
        for (int i = 0; i < n; i++) count += crowd[i].val == 2;
        *n_crowded = count;
    }
    return KLT_OK;
}

}  // extern "C"
