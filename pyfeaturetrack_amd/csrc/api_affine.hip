// api_affine.hip -- the affine consistency check behind a tracker launch: its parameters, the per-feature state (records and
// templates) and the launches.  The kernels: affine_kernels.hip.
#include "klt_context.h"

extern "C" {

int klt_set_affine_params(klt_ctx *c, const klt_affine_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode < -1 || p->mode > 2) return fail(c, KLT_ERR_ARG, "affineConsistencyCheck must be -1, 0, 1 or 2");
    if (p->mode >= 0 && (p->window_width < 3 || p->window_height < 3 || !(p->window_width & 1) || !(p->window_height & 1) ||
                         p->window_width > 63 || p->window_height > 63 || p->max_iterations < 1))
        return fail(c, KLT_ERR_ARG, "affine window must be odd, 3..63; max_iterations >= 1");
    if (c->ap.window_width != p->window_width || c->ap.window_height != p->window_height)
        for (AffState &a : c->aff)
            if (a.rec) return fail(c, KLT_ERR_STATE, "affine window cannot change while affine states exist");
    c->ap = *p;
    return KLT_OK;
}

int klt_affine_alloc(klt_ctx *c, int state, int n)
{
    if (!c || state < 0 || state > 4095 || n <= 0) return fail(c, KLT_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)state >= c->aff.size()) c->aff.resize(state + 1);
    AffState &a = c->aff[state];
    const int tn = (c->ap.window_width + 2) * (c->ap.window_height + 2);
    if (a.n < n || a.tn != tn) {
        if (a.rec) { if (int rc = sync_all(c)) return rc; hipFree(a.rec); hipFree(a.tpl); a.rec = nullptr; a.tpl = nullptr; a.n = 0; }
        DEVALLOC(c, a.rec, (size_t)n * sizeof(klt_affine_rec));
        if (int rc = dev_alloc(c, (void **)&a.tpl, (size_t)n * 3 * tn * sizeof(float), "affine templates")) {
            hipFree(a.rec);                                   // a state is its records AND its templates, or nothing
            a.rec = nullptr;
            return rc;
        }
        a.n = n;
        a.tn = tn;
    }
    launch_affine_reset(c->stream, a.rec, a.n);
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_affine_free(klt_ctx *c, int state)
{
    if (!c) return KLT_ERR_ARG;
    if (state < 0 || (size_t)state >= c->aff.size() || !c->aff[state].rec) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = sync_all(c)) return rc;
    AffState &a = c->aff[state];
    hipFree(a.rec); hipFree(a.tpl);
    a = AffState();
    if (c->select_aff_state == state) c->select_aff_state = -1;
    return KLT_OK;
}

// records (and, if asked, templates) of the first n features of `src` into `dst` (allocated here if needed), on the context's stream:
// a snapshot of the per-feature state, e.g. to replay a step of a sequence from the same state
int klt_affine_copy_async(klt_ctx *c, int dst, int src, int n, int with_templates)
{
    if (!c || dst == src || n <= 0) return fail(c, KLT_ERR_ARG, "bad argument");
    if (src < 0 || (size_t)src >= c->aff.size() || !c->aff[src].rec || c->aff[src].n < n)
        return fail(c, KLT_ERR_STATE, "source affine state not allocated (or smaller than requested)");
    if (dst < 0 || (size_t)dst >= c->aff.size() || !c->aff[dst].rec || c->aff[dst].n < n) {
        if (int rc = klt_affine_alloc(c, dst, c->aff[src].n)) return rc;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const AffState &s = c->aff[src];
    AffState &d = c->aff[dst];
    if (d.tn != s.tn) return fail(c, KLT_ERR_STATE, "affine states of different window sizes");
    HIPCHK(c, hipMemcpyAsync(d.rec, s.rec, (size_t)n * sizeof(klt_affine_rec), hipMemcpyDeviceToDevice, c->stream));
    if (with_templates)
        HIPCHK(c, hipMemcpyAsync(d.tpl, s.tpl, (size_t)n * 3 * s.tn * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return KLT_OK;
}

int klt_affine_download(klt_ctx *c, int state, klt_affine_rec *dst, int n)
{
    if (!c || !dst || state < 0 || (size_t)state >= c->aff.size() || !c->aff[state].rec || c->aff[state].n < n)
        return fail(c, KLT_ERR_STATE, "affine state not allocated (or smaller than requested)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, c->aff[state].rec, (size_t)n * sizeof(klt_affine_rec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KLT_OK;
}

int klt_track_affine_async(klt_ctx *c, int slot1, int slot2, int fb_in, int fb_out, int n, int state)
{
    if (!c) return KLT_ERR_ARG;
    if (int rc = refuse_with_light(c, "the affine consistency check")) return rc;
    if (fb_in == fb_out) return fail(c, KLT_ERR_ARG, "the consistency check needs the records before and after: fb_in != fb_out");
    if (c->ap.mode >= 0 && (state < 0 || (size_t)state >= c->aff.size() || !c->aff[state].rec || c->aff[state].n < n))
        return fail(c, KLT_ERR_STATE, "affine state not allocated (klt_affine_alloc) or smaller than the feature list");
    if (int rc = klt_track_async(c, slot1, slot2, fb_in, fb_out, n)) return rc;
    if (c->ap.mode < 0 || n == 0) return KLT_OK;
    Slot *s1 = &c->slots[slot1], *s2 = &c->slots[slot2];
    if (int rc = ensure_level0_records(c, s1)) return rc;     // (the tracker launch above may have read compact level-0 images)
    if (int rc = ensure_level0_records(c, s2)) return rc;
    AffState &as = c->aff[state];
    AffineArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = c->fbs[fb_in].d; a.out = c->fbs[fb_out].d; a.rec = as.rec; a.tpl = as.tpl;
    level_planes(s1, s2, 0, a.i1, a.gx1, a.gy1, a.i2, a.gx2, a.gy2);
    a.n = n; a.ncols = s1->nc; a.nrows = s1->nr; a.mode = c->ap.mode;
    a.width = c->ap.window_width; a.height = c->ap.window_height; a.max_iterations = c->ap.max_iterations;
    a.step = c->p.step_factor; a.small = c->p.min_determinant; a.th = c->p.min_displacement;
    a.th_aff = c->ap.min_displacement; a.max_residue = c->ap.max_residue; a.max_differ = c->ap.max_displacement_differ;
    {
        TimerScope t(c, F_AFFINE, (double)n * 12.0 * (a.width + 1) * (a.height + 1) * 3, c->stream);
        launch_affine(c->stream, a);
    }
    if (int rc = mark_read_pair(c, s1, s2)) return rc;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_track_affine(klt_ctx *c, int slot1, int slot2, klt_feat *inout, int n, int state, int *n_tracked)
{
    if (!c || !inout) return fail(c, KLT_ERR_ARG, "null argument");
    if (int rc = refuse_with_light(c, "the affine consistency check")) return rc;
    if (int rc = klt_featbuf_upload(c, kFbSyncIn, inout, n)) return rc;
    if (int rc = klt_track_affine_async(c, slot1, slot2, kFbSyncIn, kFbSyncOut, n, state)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, inout, n)) return rc;
    if (n_tracked) *n_tracked = count_live(inout, n);
    return KLT_OK;
}

}  // extern "C"
