// api_quality.hip -- per-feature track quality (not in the reference): the single-pair, batched and synchronous
// entry points.  The rule stands in include/klt_gpu.h, the kernels in quality_kernels.hip.
#include "klt_context.h"

extern "C" {

// what a quality launch asks of one pair's feature buffers before anything is allocated: the quality records in a buffer of their own
static int check_quality_buffers(klt_ctx *c, int fb_in, int fb_out, int fb_quality)
{
    return own_index(c, fb_quality, {fb_in, fb_out}, "fb_quality must be a feature buffer", "fb_quality must be distinct from fb_in and fb_out");
}

// level 0 of a pair, its two lists (the caller has found n records in each) and its quality records (allocated by the caller)
static void fill_quality_pair(klt_ctx *c, const Slot *s1, const Slot *s2, int fb_in, int fb_out, int fb_quality, QualityPair &p)
{
    p.i1 = s1->lv[0].img;
    p.i2 = s2->lv[0].img; p.gx2 = s2->lv[0].gx; p.gy2 = s2->lv[0].gy;
    p.in = c->fbs[fb_in].d; p.out = c->fbs[fb_out].d;
    p.q = reinterpret_cast<klt_quality *>(c->fbs[fb_quality].d);
}

static int enqueue_quality(klt_ctx *c, const QualityArgs &a, int npairs)
{
    const double foot = 12.0 * (c->p.window_width + 1) * (c->p.window_width + 1);
    TimerScope t(c, F_TRACK, (double)npairs * a.n * (foot * 2 + 48), c->stream);      // booked with the tracker's launches
    if (launch_track_quality(c->stream, a)) return fail(c, KLT_ERR_ARG, "unsupported window size");
    return 0;
}

int klt_track_quality_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_out, int fb_quality, int n)
{
    if (int rc = check_ready(c)) return rc;
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (int rc = check_quality_buffers(c, fb_in, fb_out, fb_quality)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s1, *s2;
    if (int rc = check_pair(c, slot1, slot2, &s1, &s2)) return rc;
    if (n == 0) return KLT_OK;
    if (int rc = lists_set(c, {fb_in, fb_out}, n)) return rc;      // (before the quality buffer is made: a refused call allocates nothing)
    if (int rc = own_records(c, fb_quality, {fb_in, fb_out}, "fb_quality must be distinct from fb_in and fb_out")) return rc;
    FeatBuf *bq;                                             // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_quality, n, &bq)) return rc;
    QualityArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_quality_pair(c, s1, s2, fb_in, fb_out, fb_quality, a.one);
    a.n = n; a.window = c->p.window_width; a.ncols = s1->nc; a.nrows = s1->nr;
    if (int rc = enqueue_quality(c, a, 1)) return rc;
    if (int rc = mark_read_pair(c, s1, s2)) return rc;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_track_quality_batch_async(klt_ctx *c, const int *slot1, const int *slot2, const int *fb_in, const int *fb_out, const int *fb_quality,
                                  int npairs, int n)
{
    if (int rc = check_ready(c)) return rc;
    if (int rc = batch_arguments(c, {slot1, slot2, fb_in, fb_out, fb_quality}, npairs, n)) return rc;
    // (quality records that another pair of the launch reads as a list, or writes too: distinct from every pair's buffers)
    for (int i = 0; i < npairs; i++)
        for (int j = 0; j < npairs; j++) {
            if (int rc = check_quality_buffers(c, fb_in[j], fb_out[j], fb_quality[i])) return rc;
            if (i != j && fb_quality[i] == fb_quality[j]) return fail(c, KLT_ERR_ARG, "two pairs of the batch share fb_quality");
        }
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<Slot *> used;
    for (int i = 0; i < npairs; i++) {
        if (int rc = batch_pair(c, slot1[i], slot2[i], false, used, true)) return rc;
        if (int rc = lists_set(c, {fb_in[i], fb_out[i]}, n)) return rc;
    }
    if (int rc = ensure_level0_records(c, used.data(), (int)used.size())) return rc;      // (lean slots: their records, one launch for all)
    if (n == 0) return KLT_OK;
    // ... and by address
    for (int i = 0; i < npairs; i++)
        for (int j = 0; j < npairs; j++)
            if (int rc = own_records(c, fb_quality[i], {fb_in[j], fb_out[j], i != j ? fb_quality[j] : -1},
                                     "fb_quality must be distinct from every pair's fb_in, fb_out and fb_quality"))
                return rc;
    for (int i = 0; i < npairs; i++) {
        FeatBuf *bq;                                         // may grow c->fbs: do it before taking pointers into it
        if (int rc = get_fb(c, fb_quality[i], n, &bq)) return rc;
    }
    std::vector<QualityPair> table((size_t)npairs);
    for (int i = 0; i < npairs; i++) {
        std::memset(&table[i], 0, sizeof(QualityPair));
        fill_quality_pair(c, used[2 * i], used[2 * i + 1], fb_in[i], fb_out[i], fb_quality[i], table[i]);
    }
    QualityArgs a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = send_if_changed(c, c->quality_table, table, &a.pairs)) return rc;
    a.npairs = npairs;
    a.n = n; a.window = c->p.window_width; a.ncols = used[0]->nc; a.nrows = used[0]->nr;
    if (int rc = enqueue_quality(c, a, npairs)) return rc;
    if (int rc = mark_read(c, used.data(), (int)used.size())) return rc;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_track_quality(klt_ctx *c, int slot1, int slot2, const klt_feat *in, const klt_feat *out, klt_quality *q, int n)
{
    if (!c || !in || !out || !q) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, in, n)) return rc;      // (the download below synchronises: both lists are ours until then)
    if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_track_quality_async(c, slot1, slot2, kFbSyncIn, kFbSyncOut, kFbSyncOwn, n)) return rc;
    if (n == 0) return klt_sync(c);
    return klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(q), n);
}

}  // extern "C"
