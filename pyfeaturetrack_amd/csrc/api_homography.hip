// api_homography.hip -- the homography check (not in the reference): parameters, the single-pair, batched and
// synchronous entry points, and the host-side change of coordinates that turns a model record into a homography in pixels.  The rule
// stands in include/klt_gpu.h, the kernels in homography_kernels.hip; the candidates come from the motion-model check's gather launch,
// and the refusals, the scratch layout and the pair descriptors from consensus_prepare* (api_model.hip).
#include "klt_context.h"
#include <cmath>

static ConsensusCheck homography_check(klt_ctx *c)
{
    return ConsensusCheck{c->hom_scratch, c->hom_scratch_cap, c->homp.hypotheses, 6, c->homp.mode != 0,
                          "the homography check is off (klt_set_homography_params mode 0)"};
}

static void fill_homography_args(const klt_ctx *c, int n, EpipolarArgs &e)
{
    const klt_homography_params &p = c->homp;
    ModelArgs &a = e.m;
    a.n = n; a.ncols = p.ncols; a.nrows = p.nrows; a.hypotheses = p.hypotheses; a.min_inliers = p.min_inliers; a.seed = p.seed;
    a.cx = (double)(p.ncols / 2); a.cy = (double)(p.nrows / 2);
    e.s = working_scale(p.ncols, p.nrows);
    const double ts = (double)p.max_error * e.s;
    a.t2 = ts * ts;
}

// the three launches, each timed as a tracker-family launch of its own (klt_timing_enable: their sum is the check's cost)
static int enqueue_homography(klt_ctx *c, const EpipolarArgs &e, int npairs)
{
    const double list = (double)npairs * e.m.n * 32;
    { TimerScope t(c, F_TRACK, list + (double)npairs * e.m.n * 40, c->stream); launch_model_gather(c->stream, e.m); }
    { TimerScope t(c, F_TRACK, list * e.m.hypotheses, c->stream); launch_homography_score(c->stream, e); }
    { TimerScope t(c, F_TRACK, list * 2, c->stream); launch_homography_decide(c->stream, e); }
    return 0;
}

extern "C" {

int klt_set_homography_params(klt_ctx *c, const klt_homography_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 0 && p->mode != 1) return fail(c, KLT_ERR_ARG, "homography mode must be 0 (off) or 1 (on)");
    if (p->hypotheses < 1 || p->hypotheses > 65536) return fail(c, KLT_ERR_ARG, "homography check: hypotheses must lie in 1 .. 65536");
    if (p->min_inliers < 4) return fail(c, KLT_ERR_ARG, "homography check: min_inliers must be at least 4");
    if (!(p->max_error >= 0.f)) return fail(c, KLT_ERR_ARG, "homography check: max_error must be a number >= 0");   // (NaN fails the comparison)
    if (p->mode == 1 && (p->ncols < 1 || p->ncols > 65535 || p->nrows < 1 || p->nrows > 65535))
        return fail(c, KLT_ERR_ARG, "homography check: ncols and nrows must lie in 1 .. 65535");
    c->homp = *p;
    return KLT_OK;
}

int klt_homography_check_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->hom_path;
}

int klt_homography_check_async(klt_ctx *c, int fb_in, int fb_out, int fb_model, int n)
{
    if (!c) return KLT_ERR_ARG;
    EpipolarArgs e;
    std::memset(&e, 0, sizeof(e));
    int go;
    if (int rc = consensus_prepare(c, homography_check(c), fb_in, fb_out, fb_model, n, &e.m.one, &go)) return rc;
    if (!go) return KLT_OK;
    fill_homography_args(c, n, e);
    if (int rc = enqueue_homography(c, e, 1)) return rc;
    c->hom_path = 1;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_homography_check_batch_async(klt_ctx *c, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n)
{
    if (!c) return KLT_ERR_ARG;
    std::vector<ModelPair> table;
    int go;
    if (int rc = consensus_prepare_batch(c, homography_check(c), fb_in, fb_out, fb_model, npairs, n, &table, &go)) return rc;
    if (!go) return KLT_OK;
    EpipolarArgs e;
    std::memset(&e, 0, sizeof(e));
    if (int rc = send_if_changed(c, c->hom_table, table, &e.m.pairs)) return rc;
    e.m.npairs = npairs;
    fill_homography_args(c, n, e);
    if (int rc = enqueue_homography(c, e, npairs)) return rc;
    c->hom_path = 2;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_homography_check(klt_ctx *c, const klt_feat *in, klt_feat *out, klt_homography_model *model, int n, int *n_outliers)
{
    if (!c || !in || !out || !model) return fail(c, KLT_ERR_ARG, "null argument");
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (c->homp.mode == 0) return fail(c, KLT_ERR_STATE, homography_check(c).off_message);
    std::memset(model, 0, sizeof(*model));
    if (n_outliers) *n_outliers = 0;
    if (n == 0) return KLT_OK;
    int before = 0;
    for (int i = 0; i < n; i++) before += out[i].val == KLT_HOMOGRAPHY_OUTLIER;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, in, n)) return rc;      // (the downloads below synchronise: both lists are ours until then)
    if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_homography_check_async(c, kFbSyncIn, kFbSyncOut, kFbSyncOwn, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(model), 6)) return rc;
    if (n_outliers) {
        int after = 0;
        for (int i = 0; i < n; i++) after += out[i].val == KLT_HOMOGRAPHY_OUTLIER;
        *n_outliers = after - before;
    }
    return KLT_OK;
}

int klt_homography_matrix(const klt_homography_model *m, double H[9])
{
    if (!m || !H) return KLT_ERR_ARG;
    if (m->valid == 0) return KLT_ERR_STATE;
    const int ncols = (int)((uint32_t)m->pad & 0xffffu), nrows = (int)((uint32_t)m->pad >> 16);
    const double s = working_scale(ncols, nrows), r = 1.0 / s;                  // (r = 2^k: exact)
    const double cx = (double)(ncols / 2), cy = (double)(nrows / 2);
    const double u = -(s * cx), v = -(s * cy);
    const double *h = m->h;
    // G = h T, then P = T^-1 G, T = [[s, 0, u], [0, s, v], [0, 0, 1]], T^-1 = [[r, 0, cx], [0, r, cy], [0, 0, 1]]
    double G[9], P[9];
    for (int i = 0; i < 3; i++) {
        G[3 * i] = s * h[3 * i];
        G[3 * i + 1] = s * h[3 * i + 1];
        G[3 * i + 2] = (h[3 * i] * u + h[3 * i + 1] * v) + h[3 * i + 2];
    }
    for (int j = 0; j < 3; j++) {
        P[j] = r * G[j] + cx * G[6 + j];
        P[3 + j] = r * G[3 + j] + cy * G[6 + j];
        P[6 + j] = G[6 + j];
    }
    double nrm = 0.0;
    for (int i = 0; i < 9; i++) nrm = nrm + P[i] * P[i];
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0) || std::isinf(nrm)) return KLT_ERR_STATE;
    if (h[8] < 0.0) nrm = -nrm;                                                 // the third coordinate positive at the image centre
    for (int i = 0; i < 9; i++) H[i] = P[i] / nrm;
    return KLT_OK;
}

}  // extern "C"
