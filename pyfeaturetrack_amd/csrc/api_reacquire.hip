// api_reacquire.hip -- track identities over a sequence (not in the reference): a persistent id per slot, a ring
// bank of what lost tracks left behind, re-acquisition of the newly selected features against it.  The rule stands in include/klt_gpu.h
// ("track identities"), the kernels in reacquire_kernels.hip; the descriptors come from the describe launch of api_describe.hip.
#include "klt_context.h"

namespace {

const char *const kIdentNoBuffer = "fb_ident must be a feature buffer";
const char *const kIdentNotDistinct = "fb_ident must be distinct from fb_list and fb_ident_prev";
const char *const kReserved = "feature buffers 29990 and 29991 hold the descriptors of the track identities";

size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// the context's one allocation for n slots and a bank of C entries, and where its parts begin
struct ReacqLayout {
    size_t bank, state, fresh_desc, fresh_slot, bank_best, fresh_best, bytes;
    ReacqLayout(int n, int C)
    {
        bank = 0;
        state = bank + (size_t)C * sizeof(klt_bank_entry);
        fresh_desc = state + 64;
        fresh_slot = fresh_desc + (size_t)n * sizeof(klt_descriptor);
        bank_best = round16(fresh_slot + (size_t)n * sizeof(int));
        fresh_best = bank_best + (size_t)C * sizeof(int4);
        bytes = fresh_best + (size_t)n * sizeof(int4);
    }
};

bool reserved(int fb) { return fb == kFbReacqDesc[0] || fb == kFbReacqDesc[1]; }

// a begin (fb_prev < 0) or a step
int reacquire_call(klt_ctx *c, int slot, int fb_list, int fb_prev, int fb_ident, int n)
{
    const bool begin = fb_prev < 0;
    // refusals
    if (n < 1) return fail(c, KLT_ERR_ARG, "track identities take at least one feature");
    if (int rc = own_index(c, fb_ident, {fb_list, fb_prev}, kIdentNoBuffer, kIdentNotDistinct)) return rc;
    if (reserved(fb_list) || reserved(fb_ident) || reserved(fb_prev)) return fail(c, KLT_ERR_ARG, kReserved);
    if (!begin) {
        if (c->reacq_n < 0) return fail(c, KLT_ERR_STATE, "klt_reacquire_step_async without klt_reacquire_begin_async");
        if (n != c->reacq_n) return fail(c, KLT_ERR_STATE, "the feature count differs from the begin call's");
    }
    const int into = begin ? 0 : 1 - c->reacq_cur;           // the descriptor buffer this call fills (Q; a begin's P)
    Slot *s;
    if (int rc = describe_refusals(c, slot, fb_list, kFbReacqDesc[into], n, &s)) return rc;
    if (!begin)
        if (int rc = lists_set(c, {fb_prev}, n)) return rc;
    if (int rc = own_records(c, fb_ident, {fb_list, fb_prev}, kIdentNotDistinct)) return rc;
    if (fb_holds(c, fb_ident, 0) && c->fbs[fb_ident].view && c->fbs[fb_ident].cap < n)
        return fail(c, KLT_ERR_ARG, "feature buffer is a view and too small");
    // allocations (a step finds everything there: the begin made it)
    const int C = begin ? c->reacqp.capacity : c->reacq_capacity;
    const ReacqLayout lay(n, C);
    if (begin) c->reacq_n = -1;                              // (a begin that fails leaves no sequence behind)
    if (int rc = ensure(c, c->reacq_mem, c->reacq_mem_cap, lay.bytes)) return rc;
    FeatBuf *b;                                              // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_ident, n, &b)) return rc;
    for (int k = 0; k < 2; k++)
        if (int rc = get_fb(c, kFbReacqDesc[k], 3 * n, &b)) return rc;
    // launches: the describe launch first (its own allocations -- the pattern, the copies of the ingest chain -- come before it)
    if (int rc = describe_enqueue(c, s, fb_list, kFbReacqDesc[into], n)) return rc;
    ReacquireArgs a;
    std::memset(&a, 0, sizeof(a));
    unsigned char *m = c->reacq_mem;
    a.list = c->fbs[fb_list].d;
    a.prev = begin ? nullptr : reinterpret_cast<const klt_ident *>(c->fbs[fb_prev].d);
    a.ident = reinterpret_cast<klt_ident *>(c->fbs[fb_ident].d);
    a.p = reinterpret_cast<const klt_descriptor *>(c->fbs[kFbReacqDesc[1 - into]].d);
    a.q = reinterpret_cast<const klt_descriptor *>(c->fbs[kFbReacqDesc[into]].d);
    a.bank = reinterpret_cast<klt_bank_entry *>(m + lay.bank);
    a.state = reinterpret_cast<int *>(m + lay.state);
    a.fresh_desc = reinterpret_cast<klt_descriptor *>(m + lay.fresh_desc);
    a.fresh_slot = reinterpret_cast<int *>(m + lay.fresh_slot);
    a.bank_best = reinterpret_cast<int4 *>(m + lay.bank_best);
    a.fresh_best = reinterpret_cast<int4 *>(m + lay.fresh_best);
    a.n = n; a.capacity = C; a.max_gap = c->reacqp.max_gap;
    a.mp = klt_match_params{c->reacqp.max_distance, c->reacqp.ratio_num, c->reacqp.ratio_den, 1, c->reacqp.radius};
    if (begin) {
        a.k = 0;
        launch_reacquire_begin(c->stream, a);
        c->reacq_n = n; c->reacq_capacity = C; c->reacq_k = 0; c->reacq_cur = 0; c->reacq_path = 2;
    } else {
        a.k = c->reacq_k + 1;
        { TimerScope t(c, F_REACQ_CLASSIFY, (double)n * (16.0 + 16.0 + 48.0) + (double)C * 64.0, c->stream); launch_reacquire_classify(c->stream, a); }
        { TimerScope t(c, F_REACQ_BANK, (double)C * 64.0, c->stream); launch_reacquire_nearest(c->stream, a, true); }
        { TimerScope t(c, F_REACQ_FRESH, (double)n * 48.0, c->stream); launch_reacquire_nearest(c->stream, a, false); }
        { TimerScope t(c, F_REACQ_ASSIGN, (double)n * 48.0, c->stream); launch_reacquire_assign(c->stream, a); }
        c->reacq_k = a.k; c->reacq_cur = into; c->reacq_path = 5;
    }
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

}  // namespace

extern "C" {

int klt_set_reacquire_params(klt_ctx *c, const klt_reacquire_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->capacity < 1 || p->capacity > 4096 || (p->capacity & (p->capacity - 1)) != 0)
        return fail(c, KLT_ERR_ARG, "reacquire capacity must be a power of two in 1 .. 4096");
    if (p->max_gap < 0) return fail(c, KLT_ERR_ARG, "reacquire max_gap must be >= 0");
    if (!match_params_ok(klt_match_params{p->max_distance, p->ratio_num, p->ratio_den, 1, p->radius}))
        return fail(c, KLT_ERR_ARG, "reacquire match parameters: max_distance 0 .. 256, ratio_num 0 or 0 < ratio_num <= ratio_den <= 65535, radius >= 0");
    c->reacqp = *p;
    c->reacq_n = -1;                                         // the sequence in progress ends: the next call must be a begin
    return KLT_OK;
}

int klt_reacquire_begin_async(klt_ctx *c, int slot, int fb_list, int fb_ident, int n)
{
    if (!c) return KLT_ERR_ARG;
    if (fb_list < 0) return fail(c, KLT_ERR_STATE, "input feature buffer not set");
    return reacquire_call(c, slot, fb_list, -1, fb_ident, n);
}

int klt_reacquire_step_async(klt_ctx *c, int slot, int fb_list, int fb_ident_prev, int fb_ident, int n)
{
    if (!c) return KLT_ERR_ARG;
    if (fb_list < 0 || fb_ident_prev < 0) return fail(c, KLT_ERR_STATE, "input feature buffer not set");
    return reacquire_call(c, slot, fb_list, fb_ident_prev, fb_ident, n);
}

int klt_reacquire_state(klt_ctx *c, struct klt_reacquire_state *st)
{
    if (!c || !st) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->reacq_n < 0) return fail(c, KLT_ERR_STATE, "no track identities have been begun");
    if (c->capturing) return fail(c, KLT_ERR_STATE, "klt_reacquire_state synchronises: not during a stream capture");
    HIPCHK(c, hipSetDevice(c->device));
    int w[kReacqStateWords];
    const ReacqLayout lay(c->reacq_n, c->reacq_capacity);
    HIPCHK(c, hipMemcpyAsync(w, c->reacq_mem + lay.state, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    st->k = c->reacq_k; st->h = w[kReacqHead]; st->next_id = w[kReacqNextId];
    st->valid = w[kReacqValid]; st->fresh = w[kReacqFresh]; st->lost = w[kReacqLost];
    return KLT_OK;
}

int klt_reacquire_download_bank(klt_ctx *c, void *entries)
{
    if (!c || !entries) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->reacq_n < 0) return fail(c, KLT_ERR_STATE, "no track identities have been begun");
    if (c->capturing) return fail(c, KLT_ERR_STATE, "klt_reacquire_download_bank synchronises: not during a stream capture");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(entries, c->reacq_mem, (size_t)c->reacq_capacity * sizeof(klt_bank_entry), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KLT_OK;
}

int klt_reacquire_path(klt_ctx *c, int *launches)
{
    if (!c || !launches) return fail(c, KLT_ERR_ARG, "null argument");
    *launches = c->reacq_path;
    return KLT_OK;
}

}  // extern "C"
