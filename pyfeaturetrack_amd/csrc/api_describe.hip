// api_describe.hip -- binary descriptors and their Hamming matcher (not in the reference): parameters, the
// asynchronous and synchronous entry points, the cut diagnostic.  The rules stand in include/klt_gpu.h, their host side (pattern, cosine
// table, the cut of the train set) in describe_rule.h, the kernels in describe_kernels.hip and match_kernels.hip.
#include "klt_context.h"
#include "describe_rule.h"

namespace {

constexpr int kMaxDescribed = 1 << 26;                       // 3 n feature records and n * splits partial results stay 32-bit counts
const char *const kDescNoBuffer = "fb_desc must be a feature buffer";
const char *const kDescNotDistinct = "fb_desc must be distinct from fb_in";
const char *const kMatchNoBuffer = "fb_match must be a feature buffer";
const char *const kMatchNotDistinct = "fb_match must be distinct from fb_query and fb_train";

// the pattern in device memory: generated and sent once per context (a synchronous copy of 1 KB)
int ensure_pattern(klt_ctx *c)
{
    if (c->desc_pattern) return 0;
    if (c->capturing) return fail(c, KLT_ERR_STATE, "the descriptor pattern would have to be sent during a stream capture");
    int8_t tests[kDescTests][4];
    desc_pattern(tests);
    int8_t *d = nullptr;
    DEVALLOC(c, d, sizeof(tests));
    if (hipError_t e = hipMemcpy(d, tests, sizeof(tests), hipMemcpyHostToDevice); e != hipSuccess) {
        hipFree(d);
        return fail(c, KLT_ERR_DEVICE, std::string("hipMemcpy (descriptor pattern): ") + hipGetErrorString(e));
    }
    c->desc_pattern = d;
    return 0;
}

}  // namespace

extern "C" {

int klt_set_descriptor_params(klt_ctx *c, const klt_descriptor_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 1 && p->mode != 2) return fail(c, KLT_ERR_ARG, "descriptor mode must be 1 (upright) or 2 (steered)");
    c->descp = *p;
    return KLT_OK;
}

}  // extern "C"

namespace kltapi {

bool match_params_ok(const klt_match_params &p)
{
    if (p.max_distance < 0 || p.max_distance > 256) return false;
    if (p.ratio_num != 0 && !(0 < p.ratio_num && p.ratio_num <= p.ratio_den && p.ratio_den <= 65535)) return false;
    return (p.cross_check == 0 || p.cross_check == 1) && p.radius >= 0;
}

int describe_refusals(klt_ctx *c, int slot, int fb_in, int fb_desc, int n, Slot **out)
{
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (n > kMaxDescribed) return fail(c, KLT_ERR_ARG, "too many features to describe in one call");
    if (int rc = own_index(c, fb_desc, {fb_in}, kDescNoBuffer, kDescNotDistinct)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    if (s->raw_kind == 0) return fail(c, KLT_ERR_STATE, "slot has no frame");
    if (s->raw_kind != 1) return fail(c, KLT_ERR_STATE, "descriptors take 8-bit frames");
    if (int rc = ingest_refusal(c, s)) return rc;
    *out = s;
    if (n == 0) return KLT_OK;
    if (int rc = lists_set(c, {fb_in}, n)) return rc;
    return own_records(c, fb_desc, {fb_in}, kDescNotDistinct);
}

int describe_enqueue(klt_ctx *c, Slot *s, int fb_in, int fb_desc, int n)
{
    // allocations: the pattern, the descriptor records (may grow c->fbs: before any pointer into it is taken), the chain's copies
    if (int rc = ensure_pattern(c)) return rc;
    FeatBuf *bd;
    if (int rc = get_fb(c, fb_desc, 3 * n, &bd)) return rc;
    // the frame, as the selection on the raw frame reads it (select_planes)
    if (int rc = wait_upload(c, s, c->stream)) return rc;
    if (int rc = wait_built(c, s)) return rc;
    if (int rc = ensure_ingested(c, &s, 1, c->stream)) return rc;
    DescribeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.frame = raw8(c, s);
    a.in = c->fbs[fb_in].d;
    a.out = reinterpret_cast<klt_descriptor *>(c->fbs[fb_desc].d);
    a.pattern = c->desc_pattern;
    a.n = n; a.ncols = s->nc; a.nrows = s->nr;
    for (int k = 0; k < kDescBins; k++) a.cs[k] = (short)kDescCos[k];
    {
        TimerScope t(c, F_DESCRIBE, (double)n * (31.0 * 31.0 + 16.0 + 48.0), c->stream);
        launch_describe(c->stream, a, c->descp.mode);
    }
    if (int rc = mark_consumed(c, &s, 1, c->stream)) return rc;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

}  // namespace kltapi

extern "C" {

int klt_describe_async(klt_ctx *c, int slot, int fb_in, int fb_desc, int n)
{
    if (!c) return KLT_ERR_ARG;
    Slot *s;
    if (int rc = describe_refusals(c, slot, fb_in, fb_desc, n, &s)) return rc;
    if (n == 0) return KLT_OK;
    return describe_enqueue(c, s, fb_in, fb_desc, n);
}

int klt_describe(klt_ctx *c, int slot, const klt_feat *in, klt_descriptor *out, int n)
{
    if (!c || !in || !out) return fail(c, KLT_ERR_ARG, "null argument");
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, in, n)) return rc;      // (the download below synchronises: the list is ours until then)
    if (int rc = klt_describe_async(c, slot, kFbSyncIn, kFbSyncOwn, n)) return rc;
    if (n == 0) return klt_sync(c);
    return klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(out), 3 * n);
}

int klt_set_match_params(klt_ctx *c, const klt_match_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (!match_params_ok(*p))
        return fail(c, KLT_ERR_ARG, "match parameters: max_distance 0 .. 256, ratio_num 0 or 0 < ratio_num <= ratio_den <= 65535, cross_check 0 or 1, radius >= 0");
    c->matchp = *p;
    return KLT_OK;
}

int klt_match_async(klt_ctx *c, int fb_query, int nq, int fb_train, int nt, int fb_match)
{
    if (!c) return KLT_ERR_ARG;
    if (nq < 0 || nt < 0) return fail(c, KLT_ERR_ARG, "negative descriptor count");
    if (nq > kMaxDescribed || nt > kMaxDescribed) return fail(c, KLT_ERR_ARG, "too many descriptors to match in one call");
    if (int rc = own_index(c, fb_match, {fb_query, fb_train}, kMatchNoBuffer, kMatchNotDistinct)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (nq == 0) return KLT_OK;
    if (int rc = lists_set(c, {fb_query}, 3 * nq)) return rc;
    if (nt > 0)
        if (int rc = lists_set(c, {fb_train}, 3 * nt)) return rc;
    if (int rc = own_records(c, fb_match, {fb_query, nt > 0 ? fb_train : -1}, kMatchNotDistinct)) return rc;
    const bool cross = c->matchp.cross_check != 0 && nt > 0;
    const int splits = match_splits(nq, nt), rsplits = cross ? match_splits(nt, nq) : 0;
    const size_t fwd = (size_t)nq * splits, bwd = (size_t)nt * rsplits;
    if (c->capturing && fwd + bwd > c->match_part_cap) return fail(c, KLT_ERR_STATE, "the match scratch would have to grow during a stream capture");
    if (int rc = ensure(c, c->match_part, c->match_part_cap, fwd + bwd)) return rc;
    FeatBuf *bm;                                             // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_match, nq, &bm)) return rc;
    const klt_descriptor *q = reinterpret_cast<const klt_descriptor *>(c->fbs[fb_query].d);
    const klt_descriptor *t = nt > 0 ? reinterpret_cast<const klt_descriptor *>(c->fbs[fb_train].d) : nullptr;
    MatchArgs m;
    std::memset(&m, 0, sizeof(m));
    m.a = q; m.na = nq; m.b = t; m.nb = nt; m.part = c->match_part; m.splits = splits; m.radius = c->matchp.radius;
    {
        TimerScope ts(c, F_MATCH, 48.0 * ((double)nq + (double)((nq + kMatchBlock - 1) / kMatchBlock) * nt), c->stream);
        launch_match(c->stream, m);
    }
    if (cross) {
        m.a = t; m.na = nt; m.b = q; m.nb = nq; m.part = c->match_part + fwd; m.splits = rsplits;
        TimerScope ts(c, F_MATCH, 48.0 * ((double)nt + (double)((nt + kMatchBlock - 1) / kMatchBlock) * nq), c->stream);
        launch_match(c->stream, m);
    }
    MatchResolveArgs r;
    std::memset(&r, 0, sizeof(r));
    r.q = q; r.fwd = c->match_part; r.bwd = cross ? c->match_part + fwd : nullptr;
    r.out = reinterpret_cast<struct klt_match *>(c->fbs[fb_match].d);
    r.nq = nq; r.nt = nt; r.splits = splits; r.rsplits = rsplits; r.p = c->matchp;
    {
        TimerScope ts(c, F_MATCH_RESOLVE, 16.0 * ((double)fwd + nq), c->stream);
        launch_match_resolve(c->stream, r);
    }
    c->match_splits = splits;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_match(klt_ctx *c, const klt_descriptor *q, int nq, const klt_descriptor *t, int nt, struct klt_match *out)
{
    if (!c || (nq > 0 && (!q || !out)) || (nt > 0 && !t)) return fail(c, KLT_ERR_ARG, "null argument");
    if (nq < 0 || nt < 0) return fail(c, KLT_ERR_ARG, "negative descriptor count");
    if (nq > kMaxDescribed || nt > kMaxDescribed) return fail(c, KLT_ERR_ARG, "too many descriptors to match in one call");
    if (nq > 0)
        if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, reinterpret_cast<const klt_feat *>(q), 3 * nq)) return rc;
    if (nq > 0 && nt > 0)
        if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, reinterpret_cast<const klt_feat *>(t), 3 * nt)) return rc;
    if (int rc = klt_match_async(c, kFbSyncIn, nq, kFbSyncOut, nt, kFbSyncOwn)) return rc;
    if (nq == 0) return klt_sync(c);
    return klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(out), nq);
}

int klt_match_path(klt_ctx *c, int *splits)
{
    if (!c || !splits) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->match_splits == 0) return fail(c, KLT_ERR_STATE, "no match has been enqueued yet");
    *splits = c->match_splits;
    return KLT_OK;
}

}  // extern "C"
