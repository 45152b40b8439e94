// api_epipolar.hip -- the epipolar check (not in the reference): parameters, the single-pair, batched and synchronous
// entry points, and the host-side change of coordinates that turns a model record into a fundamental matrix in pixels.  The rule stands
// in include/klt_gpu.h, the kernels in epipolar_kernels.hip; the candidates come from the motion-model check's gather launch, and the
// refusals, the scratch layout and the pair descriptors from consensus_prepare* (api_model.hip).
#include "klt_context.h"
#include <cmath>

static ConsensusCheck epipolar_check(klt_ctx *c)
{
    return ConsensusCheck{c->epi_scratch, c->epi_scratch_cap, c->epip.hypotheses, 6, c->epip.mode != 0,
                          "the epipolar check is off (klt_set_epipolar_params mode 0)"};
}

static void fill_epipolar_args(const klt_ctx *c, int n, EpipolarArgs &e)
{
    const klt_epipolar_params &p = c->epip;
    ModelArgs &a = e.m;
    a.n = n; a.ncols = p.ncols; a.nrows = p.nrows; a.hypotheses = p.hypotheses; a.min_inliers = p.min_inliers; a.seed = p.seed;
    a.cx = (double)(p.ncols / 2); a.cy = (double)(p.nrows / 2);
    e.s = working_scale(p.ncols, p.nrows);
    const double ts = (double)p.max_error * e.s;
    a.t2 = ts * ts;
}

// the three launches, each timed as a tracker-family launch of its own (klt_timing_enable: their sum is the check's cost)
static int enqueue_epipolar(klt_ctx *c, const EpipolarArgs &e, int npairs)
{
    const double list = (double)npairs * e.m.n * 32;
    { TimerScope t(c, F_TRACK, list + (double)npairs * e.m.n * 40, c->stream); launch_model_gather(c->stream, e.m); }
    { TimerScope t(c, F_TRACK, list * e.m.hypotheses, c->stream); launch_epipolar_score(c->stream, e); }
    { TimerScope t(c, F_TRACK, list * 2, c->stream); launch_epipolar_decide(c->stream, e); }
    return 0;
}

extern "C" {

int klt_set_epipolar_params(klt_ctx *c, const klt_epipolar_params *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "null argument");
    if (p->mode != 0 && p->mode != 1) return fail(c, KLT_ERR_ARG, "epipolar mode must be 0 (off) or 1 (on)");
    if (p->hypotheses < 1 || p->hypotheses > 65536) return fail(c, KLT_ERR_ARG, "epipolar check: hypotheses must lie in 1 .. 65536");
    if (p->min_inliers < 8) return fail(c, KLT_ERR_ARG, "epipolar check: min_inliers must be at least 8");
    if (!(p->max_error >= 0.f)) return fail(c, KLT_ERR_ARG, "epipolar check: max_error must be a number >= 0");     // (NaN fails the comparison)
    if (p->mode == 1 && (p->ncols < 1 || p->ncols > 65535 || p->nrows < 1 || p->nrows > 65535))
        return fail(c, KLT_ERR_ARG, "epipolar check: ncols and nrows must lie in 1 .. 65535");
    c->epip = *p;
    return KLT_OK;
}

int klt_epipolar_check_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->epi_path;
}

int klt_epipolar_check_async(klt_ctx *c, int fb_in, int fb_out, int fb_model, int n)
{
    if (!c) return KLT_ERR_ARG;
    EpipolarArgs e;
    std::memset(&e, 0, sizeof(e));
    int go;
    if (int rc = consensus_prepare(c, epipolar_check(c), fb_in, fb_out, fb_model, n, &e.m.one, &go)) return rc;
    if (!go) return KLT_OK;
    fill_epipolar_args(c, n, e);
    if (int rc = enqueue_epipolar(c, e, 1)) return rc;
    c->epi_path = 1;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_epipolar_check_batch_async(klt_ctx *c, const int *fb_in, const int *fb_out, const int *fb_model, int npairs, int n)
{
    if (!c) return KLT_ERR_ARG;
    std::vector<ModelPair> table;
    int go;
    if (int rc = consensus_prepare_batch(c, epipolar_check(c), fb_in, fb_out, fb_model, npairs, n, &table, &go)) return rc;
    if (!go) return KLT_OK;
    EpipolarArgs e;
    std::memset(&e, 0, sizeof(e));
    if (int rc = send_if_changed(c, c->epi_table, table, &e.m.pairs)) return rc;
    e.m.npairs = npairs;
    fill_epipolar_args(c, n, e);
    if (int rc = enqueue_epipolar(c, e, npairs)) return rc;
    c->epi_path = 2;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}

int klt_epipolar_check(klt_ctx *c, const klt_feat *in, klt_feat *out, klt_epipolar_model *model, int n, int *n_outliers)
{
    if (!c || !in || !out || !model) return fail(c, KLT_ERR_ARG, "null argument");
    if (n < 0) return fail(c, KLT_ERR_ARG, "negative feature count");
    if (c->epip.mode == 0) return fail(c, KLT_ERR_STATE, epipolar_check(c).off_message);
    std::memset(model, 0, sizeof(*model));
    if (n_outliers) *n_outliers = 0;
    if (n == 0) return KLT_OK;
    int before = 0;
    for (int i = 0; i < n; i++) before += out[i].val == KLT_EPIPOLAR_OUTLIER;
    if (int rc = klt_featbuf_upload_async(c, kFbSyncIn, in, n)) return rc;      // (the downloads below synchronise: both lists are ours until then)
    if (int rc = klt_featbuf_upload_async(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_epipolar_check_async(c, kFbSyncIn, kFbSyncOut, kFbSyncOwn, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOut, out, n)) return rc;
    if (int rc = klt_featbuf_download(c, kFbSyncOwn, reinterpret_cast<klt_feat *>(model), 6)) return rc;
    if (n_outliers) {
        int after = 0;
        for (int i = 0; i < n; i++) after += out[i].val == KLT_EPIPOLAR_OUTLIER;
        *n_outliers = after - before;
    }
    return KLT_OK;
}

int klt_epipolar_matrix(const klt_epipolar_model *m, double F[9])
{
    if (!m || !F) return KLT_ERR_ARG;
    if (m->valid == 0) return KLT_ERR_STATE;
    const int ncols = (int)((uint32_t)m->pad & 0xffffu), nrows = (int)((uint32_t)m->pad >> 16);
    const double s = working_scale(ncols, nrows);
    const double u = -(s * (double)(ncols / 2)), v = -(s * (double)(nrows / 2));
    const double *f = m->f;
    // H = f T, then G = T^T H, T = [[s, 0, u], [0, s, v], [0, 0, 1]]
    double H[9], G[9];
    for (int i = 0; i < 3; i++) {
        H[3 * i] = s * f[3 * i];
        H[3 * i + 1] = s * f[3 * i + 1];
        H[3 * i + 2] = (f[3 * i] * u + f[3 * i + 1] * v) + f[3 * i + 2];
    }
    for (int j = 0; j < 3; j++) {
        G[j] = s * H[j];
        G[3 + j] = s * H[3 + j];
        G[6 + j] = (u * H[j] + v * H[3 + j]) + H[6 + j];
    }
    double nrm = 0.0;
    for (int i = 0; i < 9; i++) nrm = nrm + G[i] * G[i];
    nrm = std::sqrt(nrm);
    if (!(nrm > 0.0) || std::isinf(nrm)) return KLT_ERR_STATE;
    for (int i = 0; i < 9; i++) F[i] = G[i] / nrm;
    return KLT_OK;
}

}  // extern "C"
