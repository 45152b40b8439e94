// api_model.hip -- the motion-model check (not in the reference): parameters, the single-pair, batched and
// synchronous entry points, and the host-side division that turns a model record into an affine map.  The rule stands in
// include/klt_gpu.h, the kernels in model_kernels.hip.  Also here: consensus_prepare*, what this check and the epipolar check
// (api_epipolar.hip) do alike before their launches.
#include "klt_context.h"

// a pair's slice of a consensus check's scratch: candidates (32 bytes each), their record numbers and aux (8 bytes each), one score per
// hypothesis, the candidate count; a multiple of 256 bytes
static size_t slice_bytes(int n, int hypotheses)
{
    const size_t b = (size_t)n * 32 + (size_t)n * 8 + (size_t)hypotheses * 4 + 16;
    return (b + 255) & ~(size_t)255;
}

static void fill_scratch(const ConsensusCheck &k, int i, int n, ModelPair &p)
{
    unsigned char *base = k.scratch + (size_t)i * slice_bytes(n, k.hypotheses);
    p.cand = reinterpret_cast<double *>(base);
    p.idx = reinterpret_cast<int *>(base + (size_t)n * 32);
    p.scores = reinterpret_cast<int *>(base + (size_t)n * 40);
    p.count = p.scores + k.hypotheses;
}

static const char *const kModelNoBuffer = "fb_model must be a feature buffer";
static const char *const kPairwiseDistinct = "fb_in, fb_out and fb_model must be pairwise distinct";
static const char *const kModelNotDistinct = "every fb_model must be distinct from every list and from each other";
static const char *const kOutNotDistinct = "every fb_out must be distinct from every other list";

// Everything a consensus check's single-pair entry point does before its launches: the refusals in their order, the scratch, the model
// buffer, the pair's descriptor.  *go = 0 with KLT_OK: n == 0, nothing to enqueue.
int kltapi::consensus_prepare(klt_ctx *c, ConsensusCheck k, int fb_in, int fb_out, int fb_model, int n, ModelPair *one, int *go)
{
    *go = 0;
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (int rc = own_index(c, fb_model, {fb_in, fb_out}, kModelNoBuffer, kPairwiseDistinct)) return rc;
    if (fb_in == fb_out) return fail(c, KLT_ERR_ARG, kPairwiseDistinct);
    if (!k.on) return fail(c, KLT_ERR_STATE, k.off_message);
    if (n == 0) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = lists_set(c, {fb_in, fb_out}, n)) return rc;
    if (c->fbs[fb_in].d == c->fbs[fb_out].d) return fail(c, KLT_ERR_ARG, kPairwiseDistinct);
    if (int rc = own_records(c, fb_model, {fb_in, fb_out}, kPairwiseDistinct)) return rc;
    if (int rc = ensure(c, k.scratch, k.scratch_cap, slice_bytes(n, k.hypotheses))) return rc;
    FeatBuf *bm;                                             // (may grow c->fbs: before any pointer into it is taken)
    if (int rc = get_fb(c, fb_model, k.model_records, &bm)) return rc;
    std::memset(one, 0, sizeof(*one));
    one->in = c->fbs[fb_in].d; one->out = c->fbs[fb_out].d;
    one->model = reinterpret_cast<klt_motion_model *>(c->fbs[fb_model].d);
    fill_scratch(k, 0, n, *one);
    *go = 1;
    return KLT_OK;
}

// ... and its batched entry point: the table of the launch
int kltapi::consensus_prepare_batch(klt_ctx *c, ConsensusCheck k, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n,
                            std::vector<ModelPair> *table, int *go)
{
    *go = 0;
    if (!fb_in || !fb_out || !fb_model || npairs <= 0 || npairs > 65535 || n < 0) return fail(c, KLT_ERR_ARG, "bad argument");
    // a model record that another pair of the launch reads as a list, a list that another pair rewrites: by index first ...
    for (int i = 0; i < npairs; i++)
        for (int j = 0; j < npairs; j++) {
            if (int rc = own_index(c, fb_model[i], {fb_in[j], fb_out[j], i != j ? fb_model[j] : -1}, kModelNoBuffer, kModelNotDistinct)) return rc;
            if (fb_out[i] == fb_in[j] || (i != j && fb_out[i] == fb_out[j])) return fail(c, KLT_ERR_ARG, kOutNotDistinct);
        }
    if (!k.on) return fail(c, KLT_ERR_STATE, k.off_message);
    if (n == 0) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 0; i < npairs; i++)
        if (int rc = lists_set(c, {fb_in[i], fb_out[i]}, n)) return rc;
    // ... then by address
    for (int i = 0; i < npairs; i++) {
        const klt_feat *oi = c->fbs[fb_out[i]].d;
        for (int j = 0; j < npairs; j++) {
            if (int rc = own_records(c, fb_model[i], {fb_in[j], fb_out[j], i != j ? fb_model[j] : -1}, kModelNotDistinct)) return rc;
            if (oi == c->fbs[fb_in[j]].d || (i != j && oi == c->fbs[fb_out[j]].d)) return fail(c, KLT_ERR_ARG, kOutNotDistinct);
        }
    }
    if (int rc = ensure(c, k.scratch, k.scratch_cap, (size_t)npairs * slice_bytes(n, k.hypotheses))) return rc;
    for (int i = 0; i < npairs; i++) {
        FeatBuf *bm;                                         // may grow c->fbs: do it before taking pointers into it
        if (int rc = get_fb(c, fb_model[i], k.model_records, &bm)) return rc;
    }
    table->assign((size_t)npairs, ModelPair());
    for (int i = 0; i < npairs; i++) {
        ModelPair &p = (*table)[i];
        std::memset(&p, 0, sizeof(ModelPair));
        p.in = c->fbs[fb_in[i]].d; p.out = c->fbs[fb_out[i]].d;
        p.model = reinterpret_cast<klt_motion_model *>(c->fbs[fb_model[i]].d);
        fill_scratch(k, i, n, p);
    }
    *go = 1;
    return KLT_OK;
}

static ConsensusCheck model_check(klt_ctx *c)
{
    return ConsensusCheck{c->model_scratch, c->model_scratch_cap, c->modelp.hypotheses, 5, c->modelp.mode != 0,
                          "the motion-model check is off (klt_set_model_params mode 0)"};
}

static void fill_model_args(const klt_ctx *c, int n, ModelArgs &a)
{
    const klt_model_params &m = c->modelp;
    a.n = n; a.ncols = m.ncols; a.nrows = m.nrows; a.hypotheses = m.hypotheses; a.min_inliers = m.min_inliers; a.seed = m.seed;
    a.cx = (double)(m.ncols / 2); a.cy = (double)(m.nrows / 2);
    a.t2 = (double)m.max_error * (double)m.max_error;
    a.min_area = (double)m.min_area;
}

// the three launches, each timed as a tracker-family launch of its own (klt_timing_enable: their sum is the check's cost)
static int enqueue_model(klt_ctx *c, const ModelArgs &a, int npairs)
{
    const double list = (double)npairs * a.n * 32;
    { TimerScope t(c, F_TRACK, list + (double)npairs * a.n * 40, c->stream); launch_model_gather(c->stream, a); }
    { TimerScope t(c, F_TRACK, (double)npairs * a.n * 32 * a.hypotheses, c->stream); launch_model_score(c->stream, a); }
    { TimerScope t(c, F_TRACK, (double)npairs * a.n * 64, c->stream); launch_model_decide(c->stream, a); }
    return 0;
}

extern "C" {

int klt_set_model_params(klt_ctx *c, const klt_model_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 0 && p->mode != 1) return fail(c, KLT_ERR_ARG, "motion-model mode must be 0 (off) or 1 (affine)");
    if (p->hypotheses < 1 || p->hypotheses > 65536) return fail(c, KLT_ERR_ARG, "motion model: hypotheses must lie in 1 .. 65536");
    if (p->min_inliers < 3) return fail(c, KLT_ERR_ARG, "motion model: min_inliers must be at least 3");
    if (!(p->max_error >= 0.f) || !(p->min_area >= 0.f))                                  // (NaN fails the comparison)
        return fail(c, KLT_ERR_ARG, "motion model: max_error and min_area must be numbers >= 0");
    if (p->mode == 1 && (p->ncols < 1 || p->ncols > 65535 || p->nrows < 1 || p->nrows > 65535))
        return fail(c, KLT_ERR_ARG, "motion model: ncols and nrows must lie in 1 .. 65535");
    c->modelp = *p;
    return KLT_OK;
}

int klt_motion_check_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->model_path;
}

int klt_motion_check_async(klt_ctx *c, int fb_in, int fb_out, int fb_model, int n)
{
    if (!c) return KLT_ERR_ARG;
    ModelArgs a;
    std::memset(&a, 0, sizeof(a));
    int go;
    if (int rc = consensus_prepare(c, model_check(c), fb_in, fb_out, fb_model, n, &a.one, &go)) return rc;
    if (!go) return KLT_OK;
    fill_model_args(c, n, a);
    if (int rc = enqueue_model(c, a, 1)) return rc;
    c->model_path = 1;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_motion_check_batch_async(klt_ctx *c, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n)
{
    if (!c) return KLT_ERR_ARG;
    std::vector<ModelPair> table;
    int go;
    if (int rc = consensus_prepare_batch(c, model_check(c), fb_in, fb_out, fb_model, npairs, n, &table, &go)) return rc;
    if (!go) return KLT_OK;
    ModelArgs a;
    std::memset(&a, 0, sizeof(a));
    if (int rc = send_if_changed(c, c->model_table, table, &a.pairs)) return rc;
    a.npairs = npairs;
    fill_model_args(c, n, a);
    if (int rc = enqueue_model(c, a, npairs)) return rc;
    c->model_path = 2;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_motion_check(klt_ctx *c, const klt_feat *in, klt_feat *out, klt_motion_model *model, int n, int *n_outliers)
{
    if (!c || !in || !out || !model) return fail(c, KLT_ERR_ARG, "null argument");
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (c->modelp.mode == 0) return fail(c, KLT_ERR_STATE, model_check(c).off_message);
    std::memset(model, 0, sizeof(*model));
    if (n_outliers) *n_outliers = 0;
    if (n == 0) return KLT_OK;
    int before = 0;
    for (int i = 0; i < n; i++) before += out[i].val == KLT_MODEL_OUTLIER;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, in, n)) return rc;      // (the downloads below synchronise: both lists are ours until then)
    if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_motion_check_async(c, kFbSyncIn, kFbSyncOut, kFbSyncOwn, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(model), 5)) return rc;
    if (n_outliers) {
        int after = 0;
        for (int i = 0; i < n; i++) after += out[i].val == KLT_MODEL_OUTLIER;
        *n_outliers = after - before;
    }
    return KLT_OK;
}

int klt_motion_model_affine(const klt_motion_model *m, double A[4], double t[2])
{
    if (!m || !A || !t) return KLT_ERR_ARG;
    if (m->valid == 0 || m->d == 0.0 || std::isnan(m->d)) return KLT_ERR_STATE;
    const double cx = (double)(((uint32_t)m->pad & 0xffffu) / 2), cy = (double)(((uint32_t)m->pad >> 16) / 2);
    A[0] = m->nxx / m->d; A[1] = m->nxy / m->d; A[2] = m->nyx / m->d; A[3] = m->nyy / m->d;
    t[0] = (m->ntx / m->d + cx) - (A[0] * cx + A[1] * cy);
    t[1] = (m->nty / m->d + cy) - (A[2] * cx + A[3] * cy);
    return KLT_OK;
}

}  // extern "C"
