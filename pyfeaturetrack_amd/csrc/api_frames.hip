// api_frames.hip -- frames on their way in and the pyramids built from them: taps, uploads (synchronous, asynchronous from pinned memory on
// the copy streams, adoption of frames already in device memory), pinned / device memory for callers without a HIP binding, the ingest
// chain in front of every reader of a raw 8-bit frame (remap, then CLAHE: ensure_ingested; its device-free rules: ingest_rule.h), the launch
// sequence of the pyramid build (klt_build_pyramids*), the stand-alone convolutions and the read-back of planes.
#include "klt_context.h"

namespace kltapi {

void make_taps(const double *k, int n, Taps &t)
{
    // scipy.ndimage.convolve1d: weights[::-1], then correlate1d's symmetry test (|a -+ b| <= DBL_EPSILON)
    std::memset(&t, 0, sizeof(t));
    t.n = n;
    for (int i = 0; i < n; i++) t.k[i] = k[n - 1 - i];
    t.sym = 0;
    if (n & 1) {
        const int half = n / 2;
        t.sym = 1;
        for (int ii = 1; ii <= half; ii++)
            if (std::fabs(t.k[half + ii] - t.k[half - ii]) > 2.220446049250313e-16) { t.sym = 0; break; }
        if (t.sym == 0) {
            t.sym = -1;
            for (int ii = 1; ii <= half; ii++)
                if (std::fabs(t.k[half + ii] + t.k[half - ii]) > 2.220446049250313e-16) { t.sym = 0; break; }
        }
    }
}


// ---- a slot takes or loses a frame
// (declared in klt_context.h) the one place that clears the flags of a slot's copies
void void_copies_from(Slot &s, IngestStage stage)
{
    if (stage <= INGEST_FRAME) s.pyr_valid = false;
    if (stage <= INGEST_REMAP) s.rm_valid = false;       // (so, while a stage is on, no copy behind a stale copy of it is valid)
    s.eq_valid = false;
}

void Slot::take_frame(int ncols, int nrows, int kind, bool in_raw)
{
    nc = ncols;
    nr = nrows;
    raw_kind = kind;
    f32_in_raw = in_raw;
    void_copies_from(*this, INGEST_FRAME);
}

void Slot::drop_frame()
{
    u8_ext = nullptr;
    gen = 0;
    take_frame(0, 0, 0, f32_in_raw);                     // (kind 0: none)
}

// a rule's answer (ingest_rule.h: the text of a refusal, or null) as a return code
static int refuse_arg(klt_ctx *c, const char *why) { return why ? fail(c, KLT_ERR_ARG, why) : 0; }

// What every entry point that brings a frame asks first: its pointers (`pointers`: none of them null), then the geometry it takes -- sides
// of 1 .. 65535 pixels and the rest of frame_geometry_refusal
static int check_frame(klt_ctx *c, bool pointers, int ncols, int nrows, int pitch, FrameUse use)
{
    if (!c || !pointers) return fail(c, KLT_ERR_ARG, "null argument");
    return refuse_arg(c, frame_geometry_refusal(ncols, nrows, pitch, use));
}

int upload_raw(klt_ctx *c, int slot, const void *px, int ncols, int nrows, int pitch, int kind)
{
    if (int rc = check_frame(c, px != nullptr, ncols, nrows, pitch, FRAME_UPLOADED)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot *s;
    if (int rc = get_slot(c, slot, &s, true)) return rc;
    if (s->upload_pending) {
        if (int rc = klt_upload_wait(c)) return rc;
        s->upload_pending = false;
    }
    if (int rc = wait_built(c, s)) return rc;                 // a build on the build stream may still read the old frame
    const size_t px_count = (size_t)ncols * nrows;
    s->u8_ext = nullptr;
    if (kind == 1) { if (int rc = ensure(c, s->raw.u8, s->raw.cap, px_count)) return rc; }
    else { if (int rc = ensure(c, s->f32, s->f32_cap, px_count)) return rc; }
    const size_t esz = kind == 1 ? 1 : sizeof(float);
    void *dst = kind == 1 ? (void *)s->raw.u8 : (void *)s->f32;
    if (pitch == ncols) HIPCHK(c, hipMemcpyAsync(dst, px, px_count * esz, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)ncols * esz, px, (size_t)pitch * esz, (size_t)ncols * esz, nrows,
                                    hipMemcpyHostToDevice, c->stream));
    // pageable host memory: the copy above is staged before returning, but make it explicit
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s->take_frame(ncols, nrows, kind, false);
    return 0;
}

int layout_pyramid(klt_ctx *c, Slot *s)
{
    const int L = c->p.nPyramidLevels, ss = c->p.subsampling;
    // one plane of pixel records (image, gradx, grady: KLT_PIX_STRIDE floats) per level; every level starts on a 16-byte boundary
    auto padded = [](int nc_, int nr_) { return ((size_t)nc_ * nr_ + 3) & ~(size_t)3; };
    size_t total = 0;
    int nc = s->nc, nr = s->nr;
    for (int l = 0; l < L; l++) {
        if (nc <= 0 || nr <= 0) return fail(c, KLT_ERR_ARG, "image too small for the requested pyramid");
        total += padded(nc, nr);
        nc /= ss;
        nr /= ss;
    }
    if (3 * total > s->planes_cap) {
        if (s->planes) { if (int rc = sync_all(c)) return rc; hipFree(s->planes); s->planes = nullptr; s->planes_cap = 0; }
        s->pyr_valid = false;                              // (the old planes are gone whether or not the new ones can be had)
        DEVALLOC(c, s->planes, 3 * total * sizeof(float));
        s->planes_cap = 3 * total;
    }
    size_t off = 0;
    nc = s->nc;
    nr = s->nr;
    for (int l = 0; l < L; l++) {
        s->lv[l].nc = nc;
        s->lv[l].nr = nr;
        s->lv[l].img = s->planes + KLT_PIX_STRIDE * off;           // the three values of a pixel side by side (klt_internal.h)
        s->lv[l].gx = s->lv[l].img + 1;
        s->lv[l].gy = s->lv[l].img + 2;
        off += padded(nc, nr);
        nc /= ss;
        nr /= ss;
    }
    s->nlev = L;
    s->ss = ss;
    return 0;
}

// slots of one frame size share a launch (for_each_group, ingest_rule.h: KLT_MAX_BATCH at a time)
static bool same_size(const Slot *a, const Slot *b) { return a->nc == b->nc && a->nr == b->nr; }

// ---- the ingest chain: remap (klt_set_remap), then CLAHE (klt_set_equalize_params); the rules: include/klt_gpu.h, DESIGN.md 9l and 9m
// What a stage is to the chain's skeleton (ensure_ingested), to the host-frame calls (host_frame_through) and to the downloads
struct IngestStep {
    IngestStage stage, reads;         // the point of the chain it makes, and the one whose output (ingest_output) it reads
    uint8_t *Slot::*buf;              // the slot's copy behind this stage, ...
    size_t Slot::*cap;                // ... its capacity in bytes ...
    bool Slot::*valid;                // ... and whether it was made from the frame the slot holds under what the context holds now
    int klt_ctx::*path;               // klt_remap_path / klt_equalize_path
    // the stage's own refusals: of a frame that is not an 8-bit one, of a launch during a stream capture, and of a frame's size --
    // when_stale: only where a launch would be needed (a valid copy is not examined again)
    const char *not_u8, *in_capture;
    int (*check)(klt_ctx *, int nc, int nr);
    bool when_stale;
    size_t (*bytes)(const klt_ctx *, int nc, int nr);      // of the copy, with whatever the stage keeps behind it
    // the launches, under their timing families, on `batch` frames of nc x nr pixels whose rows lie src_pitch bytes apart
    void (*enqueue)(klt_ctx *, const uint8_t *const *src, int src_pitch, uint8_t *const *dst, int batch, int nc, int nr, hipStream_t);
};

// what a frame must be for the context's map: of the map's size
static int check_remappable(klt_ctx *c, int nc, int nr)
{
    if (nc != c->rmp.nc || nr != c->rmp.nr)
        return fail(c, KLT_ERR_ARG, "remapping: the frame is " + std::to_string(nc) + " by " + std::to_string(nr) + ", the map " +
                                        std::to_string(c->rmp.nc) + " by " + std::to_string(c->rmp.nr));
    return 0;
}

static size_t remap_bytes(const klt_ctx *, int nc, int nr) { return (size_t)nc * nr; }

static void enqueue_remap(klt_ctx *c, const uint8_t *const *src, int src_pitch, uint8_t *const *dst, int batch, int nc, int nr, hipStream_t st)
{
    RemapArgs a{};
    for (int b = 0; b < batch; b++) { a.src[b] = src[b]; a.dst[b] = dst[b]; }
    a.batch = batch; a.src_pitch = src_pitch;
    a.map_x = c->rmp.d; a.map_y = c->rmp.d + c->rmp.plane;
    a.ncols = nc; a.nrows = nr;                            // (the map's size: check_remappable)
    TimerScope t(c, F_REMAP, (double)nc * nr * (8.0 + 2.0 * batch), st);
    launch_remap(st, a);
}

// what a frame must be for the context's tile grid (equalisable_refusal, ingest_rule.h)
static int check_equalisable(klt_ctx *c, int nc, int nr) { return refuse_arg(c, equalisable_refusal(nc, nr, c->eqp.tiles_x, c->eqp.tiles_y)); }

static size_t equalize_bytes(const klt_ctx *c, int nc, int nr) { return eq_bytes(nc, nr, c->eqp.tiles_x, c->eqp.tiles_y); }

// the two launches; a frame's LUTs lie behind its equalised copy (eq_lut_offset)
static void enqueue_equalize(klt_ctx *c, const uint8_t *const *src, int src_pitch, uint8_t *const *dst, int batch, int nc, int nr, hipStream_t st)
{
    EqualizeArgs a{};
    for (int b = 0; b < batch; b++) { a.src[b] = src[b]; a.dst[b] = dst[b]; a.lut[b] = dst[b] + eq_lut_offset(nc, nr); }
    a.src_pitch = src_pitch;
    a.ncols = nc; a.nrows = nr;
    a.tiles_x = c->eqp.tiles_x; a.tiles_y = c->eqp.tiles_y; a.clip_q8 = c->eqp.clip_q8;
    a.split = eq_apply_split(nr, a.tiles_y, batch);
    const double N = (double)nc * nr * batch;
    {
        TimerScope t(c, F_EQ_LUT, N + 256.0 * a.tiles_x * a.tiles_y * batch, st);
        launch_clahe_lut(st, a, batch);
    }
    {
        TimerScope t(c, F_EQ_APPLY, 2 * N, st);
        launch_clahe_apply(st, a, batch);
    }
}

// The two stages, in the order they run
static const IngestStep kRemapStep = {INGEST_REMAP, INGEST_FRAME, &Slot::rm, &Slot::rm_cap, &Slot::rm_valid, &klt_ctx::rm_path, "remapping takes 8-bit frames",
                                      "a frame would have to be remapped during a stream capture", check_remappable, false, remap_bytes, enqueue_remap};
static const IngestStep kEqualizeStep = {INGEST_EQUALIZE, INGEST_REMAP, &Slot::eq, &Slot::eq_cap, &Slot::eq_valid, &klt_ctx::eq_path, "equalisation takes 8-bit frames",
                                         "a frame would have to be equalised during a stream capture", check_equalisable, true, equalize_bytes, enqueue_equalize};

// those of them that are switched on
static int steps_on(const klt_ctx *c, const IngestStep *on[2])
{
    int n = 0;
    if (c->rmp.d) on[n++] = &kRemapStep;
    if (c->eqp.mode == 1) on[n++] = &kEqualizeStep;
    return n;
}

static int step_refusal(klt_ctx *c, const IngestStep &step, const Slot *s, bool stale)
{
    if (s->raw_kind != 1) return fail(c, KLT_ERR_STATE, step.not_u8);
    return stale || !step.when_stale ? step.check(c, s->nc, s->nr) : 0;
}

// (declared in klt_context.h) each stage reads the output of the last stage in front of it that is switched on
const uint8_t *ingest_output(const klt_ctx *c, const Slot *s, IngestStage upto)
{
    const IngestStep *on[2];
    const uint8_t *out = frame8(s);
    for (int k = 0, steps = steps_on(c, on); k < steps && on[k]->stage <= upto; k++) out = s->*on[k]->buf;
    return out;
}

// (declared in klt_context.h)
int ingest_refusal(klt_ctx *c, const Slot *s)
{
    const IngestStep *on[2];
    for (int k = 0, steps = steps_on(c, on); k < steps; k++)
        if (int rc = step_refusal(c, *on[k], s, false)) return rc;
    return 0;
}

// (declared in klt_context.h)
int ensure_ingested(klt_ctx *c, Slot *const *slots, int n, hipStream_t st, bool of_build /* = false */)
{
    const IngestStep *on[2];
    const int steps = steps_on(c, on);
    if (!steps) return 0;
    // 1. every refusal of every stage, stage by stage; todo: (stage, slot) wherever the slot's copy behind the stage is stale, in that
    // order (void_copies_from keeps a copy behind a stale one stale as well; the test below does not lean on it)
    std::vector<std::pair<const IngestStep *, Slot *>> todo;
    for (int k = 0; k < steps; k++)
        for (int i = 0; i < n; i++) {
            Slot *s = slots[i];
            const bool stale = !(s->*on[k]->valid) || (k > 0 && !(s->*on[k - 1]->valid));      // (its own flag, or its source is made anew)
            if (int rc = step_refusal(c, *on[k], s, stale)) return rc;
            if (stale && c->capturing) return fail(c, KLT_ERR_STATE, on[k]->in_capture);
            if (stale) todo.push_back({on[k], s});
        }
    // 2. every allocation (a slot that gets none keeps a null pointer and its cleared flag)
    for (auto &[step, s] : todo)
        if (int rc = ensure(c, s->*step->buf, s->*step->cap, step->bytes(c, s->nc, s->nr))) return rc;
    // 3. the launches: the stale slots of one stage and one frame size together (a map set: every frame has the map's size)
    for_each_group(todo.data(), todo.size(), [](const auto &a, const auto &b) { return a.first == b.first && same_size(a.second, b.second); },
                   [&](const auto *g, int B) {
        const IngestStep &step = *g[0].first;
        const Slot *s0 = g[0].second;
        const uint8_t *src[KLT_MAX_BATCH];
        uint8_t *dst[KLT_MAX_BATCH];
        for (int b = 0; b < B; b++) { src[b] = ingest_output(c, g[b].second, step.reads); dst[b] = g[b].second->*step.buf; }
        step.enqueue(c, src, s0->nc, dst, B, s0->nc, s0->nr, st);
        return 0;
    });
    // 4. the flags: a stage's new copy is valid, the copies behind it are stale until their own stage has run (and has: it comes later in
    // todo); the build has cleared both paths before the call
    for (auto &[step, s] : todo) {
        void_copies_from(*s, step->stage);
        s->*step->valid = true;
        if (of_build) c->*step->path = 1;
    }
    return 0;
}

int enqueue_smooth_raw(klt_ctx *c, Slot *s, float *dst)
{
    const int nc = s->nc, nr = s->nr;
    const double N = (double)nc * nr;
    const Taps &g = c->gauss[0];
    {
        TimerScope t(c, F_SMOOTH_H, N * ((s->raw_kind == 1 ? 1 : 4) + 4));
        if (s->raw_kind == 1) launch_hconv_u8(c->work, raw8(c, s), nc, nr, c->tmpA, nullptr, nc, 1, 0, g, nullptr);
        else launch_hconv_f32(c->work, rawf(s), nc, nr, c->tmpA, nullptr, nc, 1, 0, g, nullptr);
    }
    {
        TimerScope t(c, F_SMOOTH_V, N * 8);
        launch_vconv(c->work, c->tmpA, nullptr, nc, nr, dst, nullptr, nr, 1, 0, g, nullptr);
    }
    return 0;
}

// KLTComputeGradients, convolve.py:226-248: gx = (deriv horizontally, gauss vertically), gy = (gauss, deriv); the compact image `img`
// and its gradients into the pixel records `rec`
int enqueue_gradients(klt_ctx *c, const float *img, int nc, int nr, float *rec)
{
    const double N = (double)nc * nr;
    {
        TimerScope t(c, F_GRAD_H, N * 12);
        launch_hconv_f32(c->work, img, nc, nr, c->tmpA, c->tmpB, nc, 1, 0, c->deriv[2], &c->gauss[2]);
    }
    {
        TimerScope t(c, F_GRAD_V, N * 16);
        launch_vconv(c->work, c->tmpA, c->tmpB, nc, nr, rec + 1, rec + 2, nr, 1, 0, c->gauss[2], &c->deriv[2], KLT_PIX_STRIDE);
        launch_put_strided(c->work, img, rec, (size_t)nc * nr, KLT_PIX_STRIDE);
    }
    return 0;
}

constexpr size_t kMaxLds = 150 * 1024;     // leave headroom below the 160 KiB of a CU

int grad_radius(const klt_ctx *c) { return (c->gauss[2].n > c->deriv[2].n ? c->gauss[2].n : c->deriv[2].n) / 2; }

bool fused_smooth_ok(const klt_ctx *c)
{
    return c->use_fused && c->gauss[0].sym == 1 && smooth_grad_lds_bytes(c->gauss[0].n / 2, grad_radius(c)) <= kMaxLds;
}
// the register-blocked kernels take per-entry geometry (levels of different size in one launch); dims must fit a short
bool merged_grad_ok(const klt_ctx *c) { return l0_taps_specialised(nullptr, c->gauss[2], c->deriv[2]); }
bool fused_grad_ok(const klt_ctx *c) { return c->use_fused && smooth_grad_lds_bytes(-1, grad_radius(c)) <= kMaxLds; }
bool fused_reduce_ok(const klt_ctx *c) { return c->use_fused && pyr_reduce_lds_bytes(c->p.subsampling, c->gauss[1].n) <= kMaxLds; }

// The plan of a level-0 or gradient launch under this context's taps and options: which kernel, which form, which grid (plan_level0)
L0Plan plan_l0(const klt_ctx *c, int batch, int kind, int nc, int nr, bool uniform /* = true */, bool want_hred /* = false */, bool want_lean /* = false */)
{
    const L0Request q = {nc, nr, batch, kind, uniform, &c->gauss[0], &c->gauss[2], &c->deriv[2], &c->gauss[1], c->p.subsampling,
                         c->fuse_hreduce, c->l0_stream, c->l0_lean_form_opt, want_hred, want_lean};
    return plan_level0(q, l0_tuning_from_env());
}

// smooth(raw frame) + gradients for up to KLT_MAX_BATCH same-sized frames in one launch, as `plan` (of plan_l0 for this batch and size) has
// it: pixel records `rec`, and (cimg, optional, not with the fused reduction) the smoothed image as compact planes as well
// plan.hred: the horizontal pass of the first reduction goes out with this launch (then c->h1 holds one H1 plane of nr x (nc / ss) floats
// per frame)
// plan.lean: a lean launch (KLT_OPT_L0_LAZY_GRAD) -- only ever a streaming kernel, i.e. one with the fused reduction: the smoothed image to
// `cimg` INSTEAD of the records
int enqueue_fused_smooth_grad(klt_ctx *c, int batch, const void *const *raw, int raw_kind, float *const *rec,
                              float *const *cimg, int nc, int nr, const L0Plan &plan)
{
    SmoothGradArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int b = 0; b < batch; b++) { a.raw[b] = raw[b]; a.rec[b] = rec[b]; a.cimg[b] = cimg ? cimg[b] : nullptr; }
    a.smooth = c->gauss[0]; a.ggauss = c->gauss[2]; a.gderiv = c->deriv[2];
    a.ncols = nc; a.nrows = nr; a.R = grad_radius(c);
    if (plan.hred) {
        const size_t plane = (size_t)nr * (nc / c->p.subsampling);
        if (int rc = ensure_h1(c, plane * batch)) return rc;
        a.reduce = c->gauss[1];
        a.h1_nc = nc / c->p.subsampling;
        for (int b = 0; b < batch; b++) a.h1[b] = c->h1 + plane * b;
    }
    const double N = (double)nc * nr * batch;
    // algorithmic bytes: smoothing b_in + 4, gradients 12 per pixel; with the fused horizontal reduction this
    // launch also consumes the reduction stage's input (4 per pixel of level 0 -- the part of 4 (N0 + N1) that no longer
    // touches HBM); pyr_vreduce is charged the stage's output, so the step total is unchanged
    // (a lean launch writes the image alone, no gradients)
    TimerScope t(c, F_SMOOTH_GRAD, N * ((raw_kind == 1 ? 1 : 4) + 4) + (plan.lean ? 0.0 : N * 12) + (plan.hred ? 4.0 * N : 0.0));
    if (int e = launch_smooth_grad(c->work, a, plan))
        return fail(c, KLT_ERR_DEVICE, std::string("smooth_grad launch: ") + hipGetErrorString((hipError_t)e));
    return 0;
}

// gradients of up to KLT_MAX_BATCH same-sized compact f32 images in one launch, into pixel records (the image copied through)
int enqueue_fused_grad(klt_ctx *c, int batch, const float *const *img, float *const *rec, int nc, int nr, bool u8_input /* = false */)
{
    SmoothGradArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int b = 0; b < batch; b++) { a.raw[b] = img[b]; a.rec[b] = rec[b]; }
    a.smooth = c->gauss[0]; a.ggauss = c->gauss[2]; a.gderiv = c->deriv[2];
    a.ncols = nc; a.nrows = nr; a.R = grad_radius(c);
    TimerScope t(c, F_GRAD, (double)nc * nr * batch * 12);
    if (int e = launch_smooth_grad(c->work, a, plan_l0(c, batch, u8_input ? 3 : 2, nc, nr)))
        return fail(c, KLT_ERR_DEVICE, std::string("gradient launch: ") + hipGetErrorString((hipError_t)e));
    return 0;
}

// KLT_OPT_L0_LAZY_GRAD: would this slot's build be lean if its launch has the form?  1 (adaptive): since its previous build -- of the
// same frame size, under the same taps and pyramid shape -- a tracker launch with a lazy form read it and nothing asked for its level-0
// records.  (A slot's first build is full.)
static bool wants_lean(const klt_ctx *c, const Slot *s)
{
    if (c->l0_lazy_grad == 2) return true;
    return c->l0_lazy_grad == 1 && s->lazy_read && !s->rec0_asked && s->built_nc == s->nc && s->built_nr == s->nr && s->built_cfg == c->cfg_gen;
}

// (declared in klt_context.h)
int ensure_level0_records(klt_ctx *c, Slot *const *slots, int n, bool asked /* = true */)
{
    std::vector<Slot *> todo;
    for (int i = 0; i < n; i++) {
        Slot *s = slots[i];
        if (asked) s->rec0_asked = true;
        if (!s->pyr_valid || s->rec0_valid || std::find(todo.begin(), todo.end(), s) != todo.end()) continue;
        if (!s->l0img_valid) return fail(c, KLT_ERR_STATE, "a built slot holds neither level-0 records nor a compact level-0 image");
        if (c->capturing) return fail(c, KLT_ERR_STATE, "level-0 records would have to be made during a stream capture");
        if (int rc = wait_built(c, s)) return rc;            // the main stream is behind the slot's build
        todo.push_back(s);
    }
    if (todo.empty()) return 0;
    hipStream_t const caller = c->work;
    // slots of one frame size share a launch, KLT_MAX_BATCH at a time
    const int rc_groups = for_each_group(todo.data(), todo.size(), same_size, [&](Slot *const *g, int B) {
        const float *img[KLT_MAX_BATCH];
        float *rec[KLT_MAX_BATCH];
        for (int b = 0; b < B; b++) { img[b] = g[b]->l0img; rec[b] = g[b]->lv[0].img; }
        c->work = c->stream;
        const int rc = enqueue_fused_grad(c, B, img, rec, g[0]->nc, g[0]->nr);
        c->work = caller;
        if (rc) return rc;
        for (int b = 0; b < B; b++) g[b]->rec0_valid = true;
        return 0;
    });
    if (rc_groups) return rc_groups;
    if (caller != c->stream) {                               // a reader on the build stream: behind the launch just enqueued
        hipEvent_t e;
        if (int rc2 = fresh_event(c, &e)) return rc2;
        HIPCHK(c, hipEventRecord(e, c->stream));
        HIPCHK(c, hipStreamWaitEvent(caller, e, 0));
    }
    return 0;
}

int ensure_level0_records(klt_ctx *c, Slot *s, bool asked /* = true */) { return ensure_level0_records(c, &s, 1, asked); }

// KLT_OPT_BUILD_STREAM, entry: a build on the build stream goes behind the main stream once, a build on the main stream behind the last
// build over there
static int enter_build_stream(klt_ctx *c, bool on_bstream)
{
    if (on_bstream) {
        if (!c->bstream) HIPCHK(c, hipStreamCreateWithFlags(&c->bstream, hipStreamNonBlocking));
        if (c->last_build_on_bstream != 1) {
            // the first build over here: behind everything on the main stream (earlier builds there share the H1 scratch)
            hipEvent_t mark;
            if (int rc = fresh_event(c, &mark)) return rc;
            HIPCHK(c, hipEventRecord(mark, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->bstream, mark, 0));
        }
        c->work = c->bstream;
    } else if (c->last_build_on_bstream == 1 && c->ev_bbuild) {
        if (event_live(c, c->bbuild_serial)) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bbuild, 0));
        else HIPCHK(c, hipStreamSynchronize(c->bstream));
    }
    return 0;
}

// ... and exit: the event that readers of these slots (and the next build on the main stream) wait for
static int leave_build_stream(klt_ctx *c, const std::vector<Slot *> &sl)
{
    hipEvent_t e;
    uint64_t serial;
    if (int rc = fresh_event(c, &e, &serial)) return rc;
    HIPCHK(c, hipEventRecord(e, c->bstream));
    for (Slot *s : sl) { s->ev_built = e; s->built_serial = serial; s->built_pending = true; }
    c->ev_bbuild = e; c->bbuild_serial = serial;
    return 0;
}

// Levels 1..L-1 of one group `g` of equal frames, from the compact planes of the scratch laid out by coff / cper (level 1 from the H1 planes
// where the level-0 launch made them: h1_fused)
static int build_upper_levels(klt_ctx *c, const std::vector<Slot *> &g, bool h1_fused, bool merged_grad, const size_t *coff, size_t cper)
{
    const int B = (int)g.size(), ss = c->p.subsampling;
    Slot *s0 = g[0];
    const float *src[KLT_MAX_BATCH];
    float *rec[KLT_MAX_BATCH];
    auto cimg_of = [&](int l, int b) { return c->cimg + cper * b + coff[l]; };
    // levels 1..L-1: smooth with the pyramid sigma, keep pixel (ss*y + ss/2, ss*x + ss/2) (pyramid.py:59-72),
    // then the gradients of the new level.  Only surviving columns / rows are evaluated.
    for (int l = 1; l < s0->nlev; l++) {
        const Level &ls = s0->lv[l - 1];
        const Level &ld = s0->lv[l];
        if (fused_reduce_ok(c)) {
            PyrReduceArgs a;
            std::memset(&a, 0, sizeof(a));
            for (int b = 0; b < B; b++) { a.src[b] = cimg_of(l - 1, b); a.dst[b] = cimg_of(l, b); }
            a.taps = c->gauss[1];
            a.src_nc = ls.nc; a.src_nr = ls.nr; a.dst_nc = ld.nc; a.dst_nr = ld.nr; a.ss = ss;
            a.log2ss = 0;
            while ((1 << a.log2ss) < ss) a.log2ss++;
            if (l == 1 && h1_fused) {
                // vertical pass only: H1 (level-0 rows x level-1 columns) -> level 1
                const size_t plane = (size_t)ls.nr * ld.nc;
                for (int b = 0; b < B; b++) a.src[b] = c->h1 + plane * b;
                TimerScope t(c, F_PYR_REDUCE, 4.0 * B * ((double)ld.nc * ld.nr));
                if (int e = launch_pyr_vreduce(c->work, a, B))
                    return fail(c, KLT_ERR_DEVICE, std::string("pyr_vreduce launch: ") + hipGetErrorString((hipError_t)e));
            } else {
                TimerScope t(c, F_PYR_REDUCE, 4.0 * B * ((double)ls.nc * ls.nr + (double)ld.nc * ld.nr));
                if (int e = launch_pyr_reduce(c->work, a, B))
                    return fail(c, KLT_ERR_DEVICE, std::string("pyr_reduce launch: ") + hipGetErrorString((hipError_t)e));
            }
        } else {
            for (int b = 0; b < B; b++) {
                {
                    TimerScope t(c, F_PYR_H, 4.0 * ((double)ls.nc * ls.nr + (double)ld.nc * ls.nr));
                    launch_hconv_f32(c->work, cimg_of(l - 1, b), ls.nc, ls.nr, c->tmpA, nullptr, ld.nc, ss, ss / 2, c->gauss[1], nullptr);
                }
                {
                    TimerScope t(c, F_PYR_V, 4.0 * ((double)ld.nc * ls.nr + (double)ld.nc * ld.nr));
                    launch_vconv(c->work, c->tmpA, nullptr, ld.nc, ls.nr, cimg_of(l, b), nullptr, ld.nr, ss, ss / 2, c->gauss[1], nullptr);
                }
            }
        }
        if (merged_grad) continue;          // gradients of all levels >= 1 go out in one launch below
        if (fused_grad_ok(c)) {
            for (int b = 0; b < B; b++) { src[b] = cimg_of(l, b); rec[b] = g[b]->lv[l].img; }
            if (int rc = enqueue_fused_grad(c, B, src, rec, ld.nc, ld.nr)) return rc;
        } else {
            for (int b = 0; b < B; b++) enqueue_gradients(c, cimg_of(l, b), ld.nc, ld.nr, g[b]->lv[l].img);
        }
    }
    if (merged_grad) {
        // one launch for the gradients of every level >= 1 of every frame: entry = (frame, level), per-entry geometry; each reads its
        // compact level image and writes the level's records
        SmoothGradArgs a;
        std::memset(&a, 0, sizeof(a));
        int e = 0;
        double bytes = 0;
        for (int l = 1; l < s0->nlev; l++)
            for (int b = 0; b < B; b++, e++) {
                a.raw[e] = cimg_of(l, b); a.rec[e] = g[b]->lv[l].img;
                a.dim_c[e] = (short)g[b]->lv[l].nc; a.dim_r[e] = (short)g[b]->lv[l].nr;
                bytes += 12.0 * g[b]->lv[l].nc * g[b]->lv[l].nr;
            }
        a.smooth = c->gauss[0]; a.ggauss = c->gauss[2]; a.gderiv = c->deriv[2];
        a.ncols = s0->lv[1].nc; a.nrows = s0->lv[1].nr; a.R = grad_radius(c);
        TimerScope t(c, F_GRAD, bytes);
        if (int er = launch_smooth_grad(c->work, a, plan_l0(c, e, 2, a.ncols, a.nrows, false)))
            return fail(c, KLT_ERR_DEVICE, std::string("gradient launch: ") + hipGetErrorString((hipError_t)er));
    }
    return 0;
}

int build_pyramids_batch(klt_ctx *c, const int *slot_ids, int n)
{
    if (int rc = check_ready(c)) return rc;
    if (!slot_ids || n <= 0) return fail(c, KLT_ERR_ARG, "empty slot list");
    HIPCHK(c, hipSetDevice(c->device));
    // KLT_OPT_BUILD_STREAM: the whole build goes to the build stream, behind everything enqueued on the main stream so far (the
    // earlier readers of these slots, synchronous uploads) -- one event each way per build.  The generic two-pass kernels share
    // scratch with the selection, so they stay on the main stream.
    WorkScope work_scope{c};
    // (Round 3 measured the level-0 kernel alone on the build stream, levels >= 1 and the tracker on the main stream -- "KLT_OPT_L0_STREAM",
    // commit 72f1f4e: bit-identical, and no faster: one context 0.0452 ms per pair against 0.0462 on one stream with two pairs per launch.
    // The level-0 kernel and the tracker are both bound by VALU issue: running side by side they take 70 us where they take 48 + 26 one
    // after the other, profiles/README.md.)
    const bool on_bstream = c->build_stream_on && c->use_fused && fused_smooth_ok(c) && fused_grad_ok(c) && fused_reduce_ok(c);
    if (int rc = enter_build_stream(c, on_bstream)) return rc;
    std::vector<Slot *> sl((size_t)n);
    std::vector<uint64_t> read_waited;
    for (int i = 0; i < n; i++) {
        if (int rc = get_slot(c, slot_ids[i], &sl[i], false)) return rc;
        if (sl[i]->raw_kind == 0) return fail(c, KLT_ERR_STATE, "slot has no frame");
        if (int rc = ingest_refusal(c, sl[i])) return rc;
        for (int j = 0; j < i; j++)
            if (sl[j] == sl[i]) return fail(c, KLT_ERR_ARG, "slot listed twice");
        if (int rc = layout_pyramid(c, sl[i])) return rc;
        if (int rc = wait_upload(c, sl[i], c->work)) return rc;      // asynchronous ingest: the frame must have landed
        if (!on_bstream) { if (int rc = wait_built(c, sl[i])) return rc; }
        else if (sl[i]->read_valid) {
            // a tracker on the main stream may still be reading the pyramids this build overwrites: wait for that launch only (a mark on
            // the whole main stream would put the build behind a tracker enqueued just before it -- the overlap the stream is for)
            // (once per launch: the slots of a batch that one launch read share its event)
            if (std::find(read_waited.begin(), read_waited.end(), sl[i]->read_serial) == read_waited.end()) {
                if (event_live(c, sl[i]->read_serial)) HIPCHK(c, hipStreamWaitEvent(c->bstream, sl[i]->ev_read, 0));
                else HIPCHK(c, hipStreamSynchronize(c->stream));
                read_waited.push_back(sl[i]->read_serial);
            }
        }
        sl[i]->read_valid = false;
    }
    c->last_build_on_bstream = on_bstream ? 1 : 0;
    // The ingest stages: the frames that have no valid copy of a stage that is on get one here, behind their uploads on the stream the
    // build runs on; the level-0 launches below read the chain's output (raw8).  The mark at the end of the build covers these readers
    // of the raw frames too.
    c->eq_path = c->rm_path = 0;
    if (int rc = ensure_ingested(c, sl.data(), n, c->work, true)) return rc;
    // groups of frames with the same geometry and input type share launches
    auto same_launch = [c](const Slot *a, const Slot *b) { return same_size(a, b) && a->raw_kind == b->raw_kind && wants_lean(c, a) == wants_lean(c, b); };
    const int rc_groups = for_each_group(sl.data(), sl.size(), same_launch, [&](Slot *const *members, int B) {
        const std::vector<Slot *> g(members, members + B);
        Slot *s0 = g[0];
        const void *raw[KLT_MAX_BATCH];
        float *rec[KLT_MAX_BATCH], *cim[KLT_MAX_BATCH];
        if (int rc = ensure_tmp(c, (size_t)s0->nc * s0->nr)) return rc;

        // level 1 comes from the H1 planes written by the level-0 kernel, or from a compact copy of level 0
        // KLT_OPT_L0_LAZY_GRAD: a group of slots that want it goes out lean where the launch is a streaming kernel's (which implies the
        // fused reduction) -- the smoothed image to the slots' compact planes, no level-0 records
        const bool fused0 = fused_smooth_ok(c);
        const L0Plan plan = plan_l0(c, B, s0->raw_kind == 1 ? 0 : 1, s0->nc, s0->nr, true, fused0 && s0->nlev > 1 && fused_reduce_ok(c), wants_lean(c, s0));
        const bool lean = plan.lean;
        // The reductions read and write compact image planes, and the gradient launches of levels >= 1 read them: scratch for the levels
        // of every frame of the group (level 0 only where something reads it), 16-byte aligned
        size_t coff[KLT_MAX_LEVELS], cper = 0;
        for (int l = 0; l < s0->nlev; l++) {
            coff[l] = cper;
            if (l > 0 || (!plan.hred && (!fused0 || s0->nlev > 1))) cper += ((size_t)s0->lv[l].nc * s0->lv[l].nr + 3) & ~(size_t)3;
        }
        if (cper) { if (int rc = ensure_cimg(c, cper * B)) return rc; }
        auto cimg_of = [&](int l, int b) { return c->cimg + cper * b + coff[l]; };

        // level 0: smoothed frame (trackFeatures.py:165-166) and its gradients (:171-172)
        if (fused0) {
            for (int b = 0; b < B && lean; b++)
                if (int rc = ensure(c, g[b]->l0img, g[b]->l0img_cap, (size_t)s0->nc * s0->nr)) return rc;
            for (int b = 0; b < B; b++) {
                raw[b] = g[b]->raw_kind == 1 ? (const void *)raw8(c, g[b]) : (const void *)rawf(g[b]);
                rec[b] = g[b]->lv[0].img;
                cim[b] = lean ? g[b]->l0img : cimg_of(0, b);
            }
            const bool copy0 = !plan.hred && s0->nlev > 1;
            if (int rc = enqueue_fused_smooth_grad(c, B, raw, s0->raw_kind, rec, copy0 || lean ? cim : nullptr, s0->nc, s0->nr, plan)) return rc;
        } else {
            for (int b = 0; b < B; b++) {
                enqueue_smooth_raw(c, g[b], cimg_of(0, b));
                enqueue_gradients(c, cimg_of(0, b), g[b]->nc, g[b]->nr, g[b]->lv[0].img);
            }
        }
        // what klt_level0_path reports: the last group's level-0 kernel, and whether its gradients of levels >= 1 are one launch
        const bool merged_grad = s0->nlev > 1 && fused_grad_ok(c) && merged_grad_ok(c) && B * (s0->nlev - 1) <= KLT_MAX_BATCH && s0->nc / s0->ss <= 32767 && s0->nr / s0->ss <= 32767;
        c->l0_path = fused0 ? plan.path : KLT_L0_TWO_PASS;
        c->l0_merged_grad = merged_grad;
        c->l0_lean = lean;
        c->l0_lean_form = plan.lean_form;
        if (int rc = build_upper_levels(c, g, plan.hred, merged_grad, coff, cper)) return rc;
        for (Slot *s : g) {
            s->pyr_valid = true; s->gen = ++c->gen_counter;
            s->rec0_valid = !lean; s->l0img_valid = lean;
            s->lazy_read = s->rec0_asked = false;
            s->built_nc = s->nc; s->built_nr = s->nr; s->built_cfg = c->cfg_gen;
        }
        return 0;
    });
    if (rc_groups) return rc_groups;
    // the next asynchronous copy into these slots waits for this build
    if (int rc = mark_consumed(c, sl.data(), n, c->work)) return rc;
    if (on_bstream) { if (int rc = leave_build_stream(c, sl)) return rc; }
    for (Slot *s : sl) s->built_on_bstream = on_bstream;
    HIPCHK(c, hipGetLastError());
    return KLT_OK;
}



int download_plane(klt_ctx *c, const float *src, int stride, size_t cnt, float *dst)
{
    float *tmp = nullptr;
    if (stride != 1) {
        DEVALLOC(c, tmp, cnt * sizeof(float));
        launch_take_strided(c->stream, src, tmp, cnt, stride);
        src = tmp;
    }
    hipError_t e = hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (tmp) hipFree(tmp);
    HIPCHK(c, e);
    return KLT_OK;
}

}  // namespace kltapi

extern "C" {

int klt_set_kernels(klt_ctx *c, int which, const double *gauss, int ng, const double *deriv, int nd)
{
    if (!c || !gauss || !deriv) return fail(c, KLT_ERR_ARG, "null argument");
    if (which < 0 || which > 2) return fail(c, KLT_ERR_ARG, "which must be 0, 1 or 2");
    if (ng < 1 || nd < 1 || ng > KLT_MAX_KERNEL_WIDTH || nd > KLT_MAX_KERNEL_WIDTH || !(ng & 1) || !(nd & 1))
        return fail(c, KLT_ERR_ARG, "tap counts must be odd and at most 71");
    Taps g, d;
    make_taps(gauss, ng, g);
    make_taps(deriv, nd, d);
    // resident pyramids (sequentialMode: tc.pyramid_last, trackFeatures.py:152-161) stay valid unless the taps really change
    const bool same = c->have_taps[which] && std::memcmp(&g, &c->gauss[which], sizeof(Taps)) == 0 &&
                      std::memcmp(&d, &c->deriv[which], sizeof(Taps)) == 0;
    if (same) return KLT_OK;
    c->gauss[which] = g;
    c->deriv[which] = d;
    c->have_taps[which] = true;
    for (Slot &s : c->slots) s.pyr_valid = false;
    c->cfg_gen++;
    return KLT_OK;
}


int klt_upload_u8(klt_ctx *c, int slot, const uint8_t *px, int ncols, int nrows, int pitch)
{
    return upload_raw(c, slot, px, ncols, nrows, pitch, 1);
}

int klt_upload_f32(klt_ctx *c, int slot, const float *px, int ncols, int nrows, int pitch)
{
    return upload_raw(c, slot, px, ncols, nrows, pitch, 2);
}

int klt_host_alloc(klt_ctx *c, size_t bytes, void **out)
{
    if (!c || !out || bytes == 0) return fail(c, KLT_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    if (int rc = host_alloc(c, &p, bytes, "klt_host_alloc")) return rc;
    c->pinned.push_back(p);
    *out = p;
    return KLT_OK;
}

int klt_host_free(klt_ctx *c, void *p)
{
    if (!c || !p) return fail(c, KLT_ERR_ARG, "bad argument");
    for (size_t i = 0; i < c->pinned.size(); i++)
        if (c->pinned[i] == p) {
            if (int rc = sync_all(c)) return rc;
            HIPCHK(c, hipHostFree(p));
            c->pinned.erase(c->pinned.begin() + (long)i);
            return KLT_OK;
        }
    return fail(c, KLT_ERR_ARG, "pointer was not allocated with klt_host_alloc");
}

// one frame from pinned host memory into the slot's other raw buffer, on one of the copy streams; esz = bytes per pixel (1: u8, 4: f32;
// pitch in pixels)
static int upload_async(klt_ctx *c, int slot, const void *px, int ncols, int nrows, int pitch, size_t esz)
{
    if (int rc = check_frame(c, px != nullptr, ncols, nrows, pitch, FRAME_UPLOADED)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipPointerAttribute_t attr;                           // the source must be pinned: a pageable copy would be staged synchronously
    if (hipPointerGetAttributes(&attr, px) != hipSuccess || attr.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return fail(c, KLT_ERR_ARG, "klt_upload_u8_async / klt_upload_f32_async need pinned host memory (klt_host_alloc)");
    }
    if (!c->cstream) HIPCHK(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    const int lane = (int)(c->upload_count++ % (unsigned)c->ncopy);                 // the two frames of a pair travel side by side
    if (lane > 0 && !c->cextra[lane - 1]) HIPCHK(c, hipStreamCreateWithFlags(&c->cextra[lane - 1], hipStreamNonBlocking));
    const hipStream_t cs = lane == 0 ? c->cstream : c->cextra[lane - 1];
    Slot *s;
    if (int rc = get_slot(c, slot, &s, true)) return rc;
    const size_t px_count = (size_t)ncols * nrows * esz;      // bytes
    // write into the buffer the build before last read (normally long finished: poll, block only if it is not)
    s->u8_ext = nullptr;
    std::swap(s->raw, s->raw_alt);
    RawBuffer &r = s->raw;
    if (int rc = ensure(c, r.u8, r.cap, px_count)) return rc;
    if (r.wr_lane >= 0 && r.wr_lane != lane) {
        // an earlier copy into this very buffer went through another copy stream (a slot uploaded twice without a build in between, an
        // upload abandoned by klt_slot_adopt_u8): this one is ordered behind it -- a copy-stream event, normally long complete
        if (event_live(c, r.wr_serial)) HIPCHK(c, hipStreamWaitEvent(cs, r.ev_wr, 0));
        else HIPCHK(c, hipStreamSynchronize(r.wr_lane == 0 ? c->cstream : c->cextra[r.wr_lane - 1]));
    }
    if (r.consumed_valid) {
        if (!event_live(c, r.consumed_serial)) {
            // the event has been re-used since: wait for the reading streams themselves (a build on the build stream reads raw frames too)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->bstream) HIPCHK(c, hipStreamSynchronize(c->bstream));
        } else {
            // poll: the build in question is at most a few launches from done, and hipEventSynchronize wakes the host 50-100 us late --
            // long enough for the queues to run dry behind it (tools/ingest_probe.py: 246 us per pair with the blocking wait)
            hipError_t q = hipEventQuery(r.ev_consumed);
            for (long spins = 0; q == hipErrorNotReady; spins++) {
                (void)hipGetLastError();                          // ("not ready" must not surface in a later hipGetLastError check)
                if (spins > 2000000) { HIPCHK(c, hipEventSynchronize(r.ev_consumed)); q = hipSuccess; break; }   // (seconds: something else is wrong)
                q = hipEventQuery(r.ev_consumed);
            }
            if (q != hipSuccess) return fail(c, KLT_ERR_DEVICE, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
        r.consumed_valid = false;
    }
    if (pitch == ncols) HIPCHK(c, hipMemcpyAsync(r.u8, px, px_count, hipMemcpyHostToDevice, cs));
    else HIPCHK(c, hipMemcpy2DAsync(r.u8, (size_t)ncols * esz, px, (size_t)pitch * esz, (size_t)ncols * esz, nrows, hipMemcpyHostToDevice, cs));
    if (int rc = fresh_event(c, &s->ev_upload, &s->upload_serial)) return rc;
    HIPCHK(c, hipEventRecord(s->ev_upload, cs));
    s->upload_pending = true;
    r.ev_wr = s->ev_upload; r.wr_serial = s->upload_serial; r.wr_lane = lane;
    s->take_frame(ncols, nrows, esz == 1 ? 1 : 2, esz != 1);
    return KLT_OK;
}

int klt_upload_u8_async(klt_ctx *c, int slot, const uint8_t *px, int ncols, int nrows, int pitch)
{
    return upload_async(c, slot, px, ncols, nrows, pitch, 1);
}

int klt_upload_f32_async(klt_ctx *c, int slot, const float *px, int ncols, int nrows, int pitch)
{
    return upload_async(c, slot, px, ncols, nrows, pitch, sizeof(float));
}

int klt_upload_wait(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->cstream) HIPCHK(c, hipStreamSynchronize(c->cstream));
    for (hipStream_t x : c->cextra) if (x) HIPCHK(c, hipStreamSynchronize(x));
    return KLT_OK;
}

int klt_device_alloc(klt_ctx *c, size_t bytes, void **out)
{
    if (!c || !out || !bytes) return fail(c, KLT_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    if (int rc = dev_alloc(c, &p, bytes, "klt_device_alloc")) return rc;
    c->dev_allocs.push_back(p);
    c->dev_alloc_bytes.push_back(bytes);
    *out = p;
    return KLT_OK;
}

int klt_device_free(klt_ctx *c, void *p)
{
    if (!c) return KLT_ERR_ARG;
    for (size_t i = 0; i < c->dev_allocs.size(); i++)
        if (c->dev_allocs[i] == p) {
            HIPCHK(c, hipSetDevice(c->device));
            if (int rc = sync_all(c)) return rc;              // a build may still read a frame adopted from it
            // slots that had adopted a frame INSIDE this allocation hold no frame any more (not the slot's own raw buffer, which may be
            // smaller than the adopted frame and holds an older image); slots adopted from other memory keep theirs
            const uint8_t *lo = (const uint8_t *)p, *hi = lo + c->dev_alloc_bytes[i];
            for (Slot &s : c->slots)
                if (s.u8_ext && s.u8_ext >= lo && s.u8_ext < hi) s.drop_frame();
            // likewise a selection mask that lives inside it (klt_set_select_mask_device): the context has no mask any more
            if (c->mask && c->mask >= lo && c->mask < hi) { c->mask = nullptr; c->mask_nc = c->mask_nr = 0; }
            hipFree(p);
            c->dev_allocs.erase(c->dev_allocs.begin() + (long)i);
            c->dev_alloc_bytes.erase(c->dev_alloc_bytes.begin() + (long)i);
            return KLT_OK;
        }
    return fail(c, KLT_ERR_ARG, "not a klt_device_alloc allocation");
}

int klt_device_write(klt_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!c || !dst || !src) return fail(c, KLT_ERR_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KLT_OK;
}

int klt_slot_adopt_u8(klt_ctx *c, int slot, const uint8_t *dev_px, int ncols, int nrows, int pitch)
{
    if (int rc = check_frame(c, dev_px != nullptr, ncols, nrows, pitch, FRAME_ADOPTED)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, dev_px) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(c, KLT_ERR_ARG, "klt_slot_adopt_u8 needs device memory");
    }
    Slot *s;
    if (int rc = get_slot(c, slot, &s, true)) return rc;
    // nothing is enqueued: the pointer is what the next build / selection of the slot reads.  Work already enqueued read the slot's
    // previous frame through its own pointer and is unaffected; a pending asynchronous upload into the slot is abandoned
    s->upload_pending = false;
    s->u8_ext = dev_px;
    s->take_frame(ncols, nrows, 1, false);
    return KLT_OK;
}

int klt_build_pyramids_async(klt_ctx *c, int slot) { return build_pyramids_batch(c, &slot, 1); }

int klt_build_pyramids_batch_async(klt_ctx *c, const int *slots, int n) { return build_pyramids_batch(c, slots, n); }


int klt_build_pyramids(klt_ctx *c, int slot)
{
    if (int rc = klt_build_pyramids_async(c, slot)) return rc;
    return klt_sync(c);
}


// -------------------------------------------------------------------------------------- inspection
int klt_level0_path(klt_ctx *c, int *merged_grad)
{
    if (!c) return KLT_ERR_ARG;
    if (c->l0_path < 0) return fail(c, KLT_ERR_STATE, "no pyramid build yet");
    if (merged_grad) *merged_grad = c->l0_merged_grad ? 1 : 0;
    return c->l0_path;
}

int klt_level0_lean_form(klt_ctx *c, int *form)
{
    if (!c || !form) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->l0_path < 0) return fail(c, KLT_ERR_STATE, "no pyramid build yet");
    *form = c->l0_lean_form;
    return KLT_OK;
}

int klt_level0_lean(klt_ctx *c, int *lean)
{
    if (!c || !lean) return fail(c, KLT_ERR_ARG, "null argument");
    if (c->l0_path < 0) return fail(c, KLT_ERR_STATE, "no pyramid build yet");
    *lean = c->l0_lean ? 1 : 0;
    return KLT_OK;
}

int klt_level_dims(klt_ctx *c, int slot, int level, int *ncols, int *nrows)
{
    if (!c) return KLT_ERR_ARG;
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    if (!s->pyr_valid || level < 0 || level >= s->nlev) return fail(c, KLT_ERR_STATE, "no such pyramid level");
    if (ncols) *ncols = s->lv[level].nc;
    if (nrows) *nrows = s->lv[level].nr;
    return KLT_OK;
}

// a plane to the host; the gradient planes are stored interleaved (klt_internal.h) and leave through a plane of their own

int klt_download_f32(klt_ctx *c, int slot, int pyramid, int level, float *dst)
{
    if (!c || !dst) return fail(c, KLT_ERR_ARG, "null argument");
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    if (!s->pyr_valid || level < 0 || level >= s->nlev || pyramid < 0 || pyramid > 2) return fail(c, KLT_ERR_STATE, "no such pyramid level");
    const Level &l = s->lv[level];
    const float *src = pyramid == 0 ? l.img : (pyramid == 1 ? l.gx : l.gy);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = wait_built(c, s)) return rc;
    if (level == 0)
        if (int rc = ensure_level0_records(c, s)) return rc;
    return download_plane(c, src, KLT_PIX_STRIDE, (size_t)l.nc * l.nr, dst);
}


// ------------------------------------------------------------------------- standalone convolutions
// _convolveSeparate, convolve.py:208-219 (SciPy branch): convolve1d along axis 1 with the horizontal taps, f32, then along axis 0 with the
// vertical taps -- ANY two tap lists (1 .. 71 taps each, odd or even, no symmetry assumed: make_taps classifies them as correlate1d does).
int klt_convolve_separate_f32(klt_ctx *c, const float *src, int ncols, int nrows, const double *horiz, int nh, const double *vert, int nv, float *dst)
{
    if (!c || !src || !dst || !horiz || !vert) return fail(c, KLT_ERR_ARG, "null argument");
    if (nh < 1 || nv < 1 || nh > KLT_MAX_KERNEL_WIDTH || nv > KLT_MAX_KERNEL_WIDTH) return fail(c, KLT_ERR_ARG, "1 to 71 taps per direction");
    if (ncols <= 0 || nrows <= 0 || (long long)ncols * nrows > kMaxFramePixels) return fail(c, KLT_ERR_ARG, "bad image geometry");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)ncols * nrows;
    if (int rc = ensure_tmp(c, N)) return rc;
    float *d_in = nullptr;
    DEVALLOC(c, d_in, 2 * N * sizeof(float));
    float *d_out = d_in + N;
    Taps th, tv;
    make_taps(horiz, nh, th);
    make_taps(vert, nv, tv);
    hipError_t e = hipMemcpyAsync(d_in, src, N * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_hconv_f32(c->stream, d_in, ncols, nrows, c->tmpA, nullptr, ncols, 1, 0, th, nullptr);
        launch_vconv(c->stream, c->tmpA, nullptr, ncols, nrows, d_out, nullptr, nrows, 1, 0, tv, nullptr);
        e = hipMemcpyAsync(dst, d_out, N * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_in);
    if (e != hipSuccess) return fail(c, KLT_ERR_DEVICE, hipGetErrorString(e));
    return KLT_OK;
}

int klt_smooth_f32(klt_ctx *c, const float *src, int ncols, int nrows, const double *gauss, int ng, float *dst)
{
    if (!c || !src || !dst || !gauss) return fail(c, KLT_ERR_ARG, "null argument");
    if (ng < 1 || ng > KLT_MAX_KERNEL_WIDTH || !(ng & 1)) return fail(c, KLT_ERR_ARG, "tap count must be odd and at most 71");
    return klt_convolve_separate_f32(c, src, ncols, nrows, gauss, ng, gauss, ng, dst);      // KLTComputeSmoothedImage, convolve.py:263
}

// ------------------------------------------------------------------------------- the ingest stages by name
// One host frame through one stage, whatever else the context has switched on: one allocation holds the frame as the caller laid it out
// and, from the next 256-byte boundary on, what the stage writes (step.bytes); the stage's ncols * nrows bytes come back.  Synchronises.
static int host_frame_through(klt_ctx *c, const IngestStep &step, const uint8_t *src, int ncols, int nrows, int pitch, uint8_t *dst)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)ncols * nrows, src_bytes = (size_t)pitch * (nrows - 1) + ncols;
    const size_t dst_off = (src_bytes + 255) & ~(size_t)255;
    uint8_t *d = nullptr;
    DEVALLOC(c, d, dst_off + step.bytes(c, ncols, nrows));
    hipError_t e = hipMemcpyAsync(d, src, src_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const uint8_t *from = d;
        uint8_t *to = d + dst_off;
        step.enqueue(c, &from, pitch, &to, 1, ncols, nrows, c->stream);
        e = hipMemcpyAsync(dst, to, N, hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    hipFree(d);
    if (e != hipSuccess) return fail(c, KLT_ERR_DEVICE, hipGetErrorString(e));
    return KLT_OK;
}

// the copy behind a stage that the slot's last build (or selection on the raw frame) read; `none`: the refusal where it holds none
static int download_stage_copy(klt_ctx *c, const IngestStep &step, int slot, uint8_t *dst, const char *none)
{
    if (!c || !dst) return fail(c, KLT_ERR_ARG, "null argument");
    Slot *s;
    if (int rc = get_slot(c, slot, &s, false)) return rc;
    if (!(s->*step.valid) || !(s->*step.buf)) return fail(c, KLT_ERR_STATE, none);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = wait_built(c, s)) return rc;                 // the stage may have run on the build stream
    HIPCHK(c, hipMemcpyAsync(dst, s->*step.buf, (size_t)s->nc * s->nr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KLT_OK;
}

// the two equalisation kernels under the context's tiles and clip limit (whatever its mode)
int klt_equalize_u8(klt_ctx *c, const uint8_t *src, int ncols, int nrows, int pitch, uint8_t *dst)
{
    if (int rc = check_frame(c, src && dst, ncols, nrows, pitch, FRAME_HOST)) return rc;
    if (int rc = check_equalisable(c, ncols, nrows)) return rc;
    return host_frame_through(c, kEqualizeStep, src, ncols, nrows, pitch, dst);
}

int klt_download_equalized_u8(klt_ctx *c, int slot, uint8_t *dst)
{
    return download_stage_copy(c, kEqualizeStep, slot, dst, "the slot holds no equalised frame (mode 0, or a new frame or new parameters since its last build)");
}

int klt_equalize_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->eq_path;
}

// the remap kernel under the context's map
int klt_remap_u8(klt_ctx *c, const uint8_t *src, int ncols, int nrows, int pitch, uint8_t *dst)
{
    if (int rc = check_frame(c, src && dst, ncols, nrows, pitch, FRAME_HOST)) return rc;
    if (!c->rmp.d) return fail(c, KLT_ERR_STATE, "no map set (klt_set_remap)");
    if (int rc = check_remappable(c, ncols, nrows)) return rc;
    return host_frame_through(c, kRemapStep, src, ncols, nrows, pitch, dst);
}

int klt_download_remapped_u8(klt_ctx *c, int slot, uint8_t *dst)
{
    return download_stage_copy(c, kRemapStep, slot, dst, "the slot holds no remapped frame (no map set, or a new frame or a new map since its last build)");
}

int klt_remap_path(klt_ctx *c)
{
    if (!c) return KLT_ERR_ARG;
    return c->rm_path;
}

int klt_gradients_f32(klt_ctx *c, const float *src, int ncols, int nrows, const double *gauss, int ng,
                      const double *deriv, int nd, float *gx, float *gy)
{
    if (!c || !src || !gx || !gy || !gauss || !deriv) return fail(c, KLT_ERR_ARG, "null argument");
    if (ng < 1 || nd < 1 || ng > KLT_MAX_KERNEL_WIDTH || nd > KLT_MAX_KERNEL_WIDTH || !(ng & 1) || !(nd & 1))
        return fail(c, KLT_ERR_ARG, "tap counts must be odd and at most 71");
    if (ncols <= 0 || nrows <= 0 || (long long)ncols * nrows > kMaxFramePixels) return fail(c, KLT_ERR_ARG, "bad image geometry");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)ncols * nrows;
    if (int rc = ensure_tmp(c, N)) return rc;
    float *d_in = nullptr;
    DEVALLOC(c, d_in, 3 * N * sizeof(float));
    float *d_gx = d_in + N, *d_gy = d_in + 2 * N;
    Taps g, d;
    make_taps(gauss, ng, g);
    make_taps(deriv, nd, d);
    hipError_t e = hipMemcpyAsync(d_in, src, N * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_hconv_f32(c->stream, d_in, ncols, nrows, c->tmpA, c->tmpB, ncols, 1, 0, d, &g);
        launch_vconv(c->stream, c->tmpA, c->tmpB, ncols, nrows, d_gx, d_gy, nrows, 1, 0, g, &d);
        e = hipMemcpyAsync(gx, d_gx, N * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(gy, d_gy, N * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_in);
    if (e != hipSuccess) return fail(c, KLT_ERR_DEVICE, hipGetErrorString(e));
    return KLT_OK;
}

// KLTPyramid.Compute, pyramid.py:37-77: level 0 = src as it is; level i = level i-1 smoothed with `gauss` (sigma = subsampling *
// sigma_fact, computed by the caller) and sampled at (ss y + ss/2, ss x + ss/2), dims int(n / ss).  Levels 1 .. nlevels-1 come back
// concatenated in dst.  Only the surviving columns / rows are evaluated; every level stays on the device until the one download.
int klt_pyramid_f32(klt_ctx *c, const float *src, int ncols, int nrows, int nlevels, int subsampling, const double *gauss, int ng, float *dst)
{
    if (!c || !src || !gauss || (nlevels > 1 && !dst)) return fail(c, KLT_ERR_ARG, "null argument");
    if (ng < 1 || ng > KLT_MAX_KERNEL_WIDTH || !(ng & 1)) return fail(c, KLT_ERR_ARG, "tap count must be odd and at most 71");
    if (ncols <= 0 || nrows <= 0 || (long long)ncols * nrows > kMaxFramePixels || nlevels < 1 || nlevels > KLT_MAX_LEVELS) return fail(c, KLT_ERR_ARG, "bad pyramid geometry");
    const int ss = subsampling;
    if (nlevels > 1 && ss != 2 && ss != 4 && ss != 8 && ss != 16 && ss != 32) return fail(c, KLT_ERR_ARG, "subsampling must be 2, 4, 8, 16 or 32");
    if (nlevels == 1) return KLT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)ncols * nrows;
    size_t total = 0;
    {
        int nc = ncols, nr = nrows;
        for (int l = 1; l < nlevels; l++) {
            nc /= ss; nr /= ss;
            if (nc <= 0 || nr <= 0) return fail(c, KLT_ERR_ARG, "image too small for the requested pyramid");
            total += (size_t)nc * nr;
        }
    }
    if (int rc = ensure_tmp(c, N)) return rc;
    float *d_in = nullptr;
    DEVALLOC(c, d_in, (N + total) * sizeof(float));
    float *d_lv = d_in + N;
    Taps g;
    make_taps(gauss, ng, g);
    hipError_t e = hipMemcpyAsync(d_in, src, N * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const float *cur = d_in;
        float *out = d_lv;
        int nc = ncols, nr = nrows;
        for (int l = 1; l < nlevels; l++) {
            const int dc = nc / ss, dr = nr / ss;
            launch_hconv_f32(c->stream, cur, nc, nr, c->tmpA, nullptr, dc, ss, ss / 2, g, nullptr);
            launch_vconv(c->stream, c->tmpA, nullptr, dc, nr, out, nullptr, dr, ss, ss / 2, g, nullptr);
            cur = out;
            out += (size_t)dc * dr;
            nc = dc; nr = dr;
        }
        e = hipMemcpyAsync(dst, d_lv, total * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_in);
    if (e != hipSuccess) return fail(c, KLT_ERR_DEVICE, hipGetErrorString(e));
    return KLT_OK;
}


}  // extern "C"
