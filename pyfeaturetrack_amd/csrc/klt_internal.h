// Internal declarations shared by the HIP translation units of libkltgpu.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "klt_gpu.h"
#include "l0_plan.h"                  // Taps, KLT_MAX_BATCH, the level-0 launch plan
#include "track_plan.h"               // the tracker launch plan, track_npad

struct SmoothGradArgs {
    const void *raw[KLT_MAX_BATCH];   // u8 or f32 frame (or, for gradients only, the compact level image)
    float *rec[KLT_MAX_BATCH];        // pixel records out (KLT_PIX_STRIDE): image, gradx, grady; gradients only: the image is copied through
    float *cimg[KLT_MAX_BATCH];       // optional (smoothing kinds, not with HRED): the smoothed image as a compact plane as well
    Taps smooth, ggauss, gderiv;
    int ncols, nrows, R;              // R = max gradient tap radius; ncols/nrows = largest entry (grid extent)
    short dim_c[KLT_MAX_BATCH], dim_r[KLT_MAX_BATCH];   // per-entry geometry when entries differ (0 = use ncols/nrows)
    // fused horizontal pass of the first pyramid reduction (smooth_grad_rb<..., HRED>): taps, H1 planes [nrows][h1_nc]
    Taps reduce;
    float *h1[KLT_MAX_BATCH];
    int h1_nc;
};

struct PyrReduceArgs {
    const float *src[KLT_MAX_BATCH];
    float *dst[KLT_MAX_BATCH];
    Taps taps;
    int src_nc, src_nr, dst_nc, dst_nr, ss, log2ss;
};

// A pyramid level is ONE plane of 12-byte pixel records: pixel (y, x) holds the image at element 3 (y nc + x), gradx right behind it
// and grady behind that, so img, gx = img + 1 and gy = img + 2 are three planes of element stride KLT_PIX_STRIDE.  A row of a tracking
// window's footprint is then one contiguous piece (96 bytes for an 8-pixel row) instead of a 32-byte piece of an image plane and a
// 64-byte piece of a gradient plane -- the tracker is bound by the cache lines its footprints touch.  Producers
// (level-0 kernels, gradient kernels) write the records, consumers (tracker, affine check, summed-area row pass) read them; only the
// plane download of the ABI separates the three planes again.  The pyramid reductions work on compact image planes in scratch
// (api_frames.hip).  The selection's own scratch uses the same records.
constexpr int KLT_PIX_STRIDE = 3;

struct TrackLevel {
    const float *i1, *gx1, *gy1, *i2, *gx2, *gy2;   // records: gx == i + 1, gy == i + 2 (KLT_PIX_STRIDE)
    int nc, nr;
};

// one frame pair of a batched tracker launch (table in device memory, indexed by blockIdx.y)
struct TrackPairDesc {
    TrackLevel lv[KLT_MAX_LEVELS];
    const klt_feat *in;
    klt_feat *out;
    klt_feat *back;                     // forward-backward launches: the backward records of the pair, or null (last: the offsets above stay)
    const klt_feat *guess;              // launches with a motion prior: the pair's predicted positions, or null (read by those kernels alone)
};

// The kernel argument of the plain tracker kernels.  Its layout is what their register allocation was measured with (the compiler widens
// scalar loads up to the end of the kernarg segment: a longer struct moved SGPR counts, a VGPR and 12 bytes of scratch), so what the
// forward-backward kernels need on top lives in TrackArgs below and the plain kernels never see it.
struct TrackArgsBase {
    TrackLevel lv[KLT_MAX_LEVELS];      // single-pair launch: levels travel in the kernarg segment
    const klt_feat *in;
    klt_feat *out;
    const TrackPairDesc *pairs;         // batched launch: npairs descriptors (lv / in / out above unused)
    int npairs;
    uint32_t *order;                    // optional: scratch [npairs][n] for the XCD-aware feature order, one permutation per pair (see track_order_kernel)
    int order_chunk;                    // ceil(n / 8): features per XCD
    int order_refresh;                  // 1: sort before this launch; 0: reuse the order of an earlier launch on the same buffer (any
                                        // permutation of 0..n-1 is correct; an old one is only a little less local)
    double half_window;          // window/2 as the Python float (3.5 for 7x7), trackFeatures.py:88-89
    double borderx, bordery;
    int n, nlevels, window, max_iterations, use_max_residue, retain, ncols, nrows;
    float small, th, step, max_residue, ss, inv_ss;
    int tree_sums;               // KLT_OPT_TRACK_TREE_SUMS: the quad kernels add the five sums (and the residue) by a butterfly in registers
};

// A tracker launch as the API describes it, and the kernel argument of the forward-backward kernels (klt_track_fb_async; DESIGN.md
// section 9a)
struct TrackArgs : TrackArgsBase {
    int fb;                      // 1: the fused forward-backward kernels (always the reference-order sums: tree_sums is not looked at)
    klt_feat *back;              // single-pair launch: the backward records, or null
    double fb_max_e2;            // (double)max_error * (double)max_error: a feature is consistent when its round trip ends within it
};

// ... and the kernel argument of the kernels that start a feature's search from a predicted position (klt_track_guess_async; DESIGN.md
// section 9c): the plain and the forward-backward kernels never see the pointer
struct TrackGuessArgs : TrackArgs {
    const klt_feat *guess;       // single-pair launch: one record per feature (x, y = predicted frame-2 position; val < 0: no guess)
};

// ... and the kernel argument of the plain 7x7 quad kernels that make their level-0 gradients themselves (KLT_OPT_L0_LAZY_GRAD; DESIGN.md
// section 5): level 0 of both frames is the slot's compact image plane (lv[0].i1 / .i2, element stride 1; the four gradient pointers of
// that level are not looked at), and the kernels carry the taps of the two gradient filters -- 7 taps each, the four left of and at the
// centre as corr_regs (below) reads them.  A struct of its own: TrackArgsBase and the kernels that take it stay as they are.
struct TrackLazyArgs : TrackArgsBase {
    double kg[4], kd[4];         // Gaussian (symmetric) and derivative (antisymmetric) taps
};

// one frame pair of a quality launch (klt_track_quality_async): level 0 of the two frames as the tracker reads it
// (records, KLT_PIX_STRIDE), the two lists and the quality records.  The table of a batched launch (device memory, indexed by
// blockIdx.y) holds these: a table of its own, TrackPairDesc stays as it is.
static_assert(sizeof(klt_quality) == sizeof(klt_feat) && alignof(klt_quality) == alignof(klt_feat), "quality records live in feature buffers");
struct QualityPair {
    const float *i1;                    // frame 1: image plane of level 0
    const float *i2, *gx2, *gy2;        // frame 2: image and gradient planes of level 0
    const klt_feat *in, *out;
    klt_quality *q;
};

struct QualityArgs {
    QualityPair one;                    // single-pair launch
    const QualityPair *pairs;           // batched launch: npairs descriptors (`one` unused)
    int npairs;
    int n, window, ncols, nrows;
};

// one frame pair of a motion-model check (klt_motion_check_async): the two lists, the model record (in a feature
// buffer of five records) and the pair's part of the context's scratch.  The table of a batched launch (device memory, indexed by
// blockIdx.y) holds these.
static_assert(sizeof(klt_motion_model) == 5 * sizeof(klt_feat), "a model record lives in a feature buffer of five records");
struct ModelPair {
    const klt_feat *in;
    klt_feat *out;
    klt_motion_model *model;
    double *cand;                       // [n][4]: (p.x, p.y, q.x, q.y) of candidate k, centred
    int *idx;                           // [n][2]: candidate k's record number and its out.aux
    int *scores;                        // [hypotheses]
    int *count;                         // m, the number of candidates
};

struct ModelArgs {
    ModelPair one;                      // single-pair launch
    const ModelPair *pairs;             // batched launch: npairs descriptors (`one` unused)
    int npairs;
    int n, ncols, nrows, hypotheses, min_inliers;
    uint32_t seed;
    double cx, cy;                      // (double)(ncols / 2), (double)(nrows / 2)
    double t2;                          // (double)max_error * (double)max_error
    double min_area;
};

// the epipolar check (klt_epipolar_check_async) gathers its candidates with the motion-model check's launch and
// descriptors (ModelPair::model then points at a klt_epipolar_model, in a feature buffer of six records; ModelArgs::min_area is unused,
// t2 is the squared threshold in working coordinates); its own two kernels also take the working scale
static_assert(sizeof(klt_epipolar_model) == 6 * sizeof(klt_feat), "an epipolar model record lives in a feature buffer of six records");
struct EpipolarArgs {
    ModelArgs m;
    double s;                           // 2^-k, k the smallest integer with 2 * (1 << k) >= max(ncols, nrows)
};
// the homography check (klt_homography_check_async) takes the same arguments: ModelPair::model then points at a
// klt_homography_model
static_assert(sizeof(klt_homography_model) == 6 * sizeof(klt_feat), "a homography model record lives in a feature buffer of six records");

// one list of a crowding check (klt_crowd_check_async): the list, the previous step's crowd records (null: none),
// this step's, and the list's part of the context's scratch.  The table of a batched launch (device memory, indexed by blockIdx.y)
// holds these.
static_assert(sizeof(klt_crowd) == sizeof(klt_feat), "crowd records live in feature buffers");
struct CrowdCand { int cell, pos, age, idx; };      // cell: -1 = no candidate; pos = px | py << 16; idx: in `info` the candidate's place in its
                                                    // cell, in `sorted` the record's number
struct CrowdPair {
    klt_feat *out;
    const klt_crowd *prev;
    klt_crowd *crowd;
    CrowdCand *info;                    // [n]: record i as the prepare launch classified it
    CrowdCand *sorted;                  // [n]: the m candidates, grouped by cell (row-major cell order; any order inside a cell)
    int *cells;                         // [gx * gy]: candidates per cell
    int *starts;                        // [gx * gy + 1]: where each cell's group begins in `sorted`; the last entry is m, the candidates
    int *state;                         // [n]: a candidate's state, for lists longer than the resolve kernel's LDS holds
    int *rounds;                        // [4]: the rounds the resolve kernel took; 10 ns ticks of its grouping, its rounds, its record writing
};
struct CrowdArgs {
    CrowdPair one;                      // single-list launch
    const CrowdPair *pairs;             // batched launch: npairs descriptors (`one` unused)
    int npairs;
    int n, ncols, nrows, r;             // r = min_distance - 1
    int side, gx, gy;                   // square cells of `side` pixels (> r: all neighbours within 3 x 3 cells), gx x gy of them
};
constexpr int kCrowdLdsStates = 24576;  // lists up to this length keep pixel and state of every candidate in LDS (5 bytes each: 120 KiB)

// the two launches of an equalisation (equalize_kernels.hip) on up to KLT_MAX_BATCH 8-bit frames of one size: the
// frames (src_pitch bytes from row to row, read only), their equalised copies (ncols bytes from row to row, 16-byte aligned) and a LUT
// buffer per frame (tiles_x * tiles_y * 256 bytes, 16-byte aligned: written by the first launch, read by the second)
struct EqualizeArgs {
    const uint8_t *src[KLT_MAX_BATCH];
    uint8_t *dst[KLT_MAX_BATCH];
    uint8_t *lut[KLT_MAX_BATCH];
    int ncols, nrows, src_pitch;
    int tiles_x, tiles_y, clip_q8;
    int split;                          // apply launch: workgroups per band of rows between two tile centres
};

// the launch of a remap (remap_kernels.hip) on `batch` (up to KLT_MAX_BATCH) 8-bit frames of one size under one
// map: the frames (src_pitch bytes from row to row, read only), their remapped copies (ncols bytes from row to row, 16-byte aligned) and
// the map as two planes of ncols * nrows int32 (1/256 px, any value; 16-byte aligned)
struct RemapArgs {
    const uint8_t *src[KLT_MAX_BATCH];
    uint8_t *dst[KLT_MAX_BATCH];
    const int32_t *map_x, *map_y;
    int ncols, nrows, src_pitch;
    int batch;
};

// the describe launch (describe_kernels.hip): the slot's 8-bit frame (ncols bytes from row to row), the list, the
// descriptor records (in a feature buffer of 3 n records), the pattern (256 tests of four int8, 4-byte aligned) and the cosine table
static_assert(sizeof(klt_descriptor) == 3 * sizeof(klt_feat) && alignof(klt_descriptor) == alignof(klt_feat), "a descriptor lives in three feature records");
static_assert(sizeof(struct klt_match) == sizeof(klt_feat) && alignof(struct klt_match) == alignof(klt_feat), "match records live in feature buffers");
struct DescribeArgs {
    const uint8_t *frame;
    const klt_feat *in;
    klt_descriptor *out;
    const int8_t *pattern;
    int n, ncols, nrows;
    short cs[32];                       // C[k]; S[k] = C[(k + 24) & 31]
};

// a match launch (match_kernels.hip): every record of `a` (na of them, one per lane) against the range blockIdx.y of `b` (nb records cut
// into `splits` ranges, describe_rule.h: match_range); part[split * na + i] = (best distance, best index or -1, second distance, 0)
struct MatchArgs {
    const klt_descriptor *a, *b;
    int4 *part;
    int na, nb, splits, radius;
};
// ... and its resolve launch: the forward partial results (nq x splits), the backward ones when the cross-check is on (nt x rsplits,
// else null), the parameters, one klt_match per query
struct MatchResolveArgs {
    const klt_descriptor *q;
    const int4 *fwd, *bwd;
    struct klt_match *out;
    int nq, nt, splits, rsplits;
    klt_match_params p;
};

// track identities (reacquire_kernels.hip).  What the context keeps in device memory for them: the bank, the
// counters (kReacq* words of `state`), the dense list of the step's fresh slots (their Q records and slot indices) and the two sets of
// nearest-neighbour results (one int4 per bank entry, one per fresh record: best distance, best index or -1, second distance, 0)
static_assert(sizeof(klt_ident) == sizeof(klt_feat) && alignof(klt_ident) == alignof(klt_feat), "ident records live in feature buffers");
static_assert(sizeof(klt_bank_entry) == 64, "a bank entry is four 16-byte pieces");
enum { kReacqNextId, kReacqHead, kReacqValid, kReacqFresh, kReacqLost, kReacqStateWords = 8 };
constexpr int kReacqBlock = 256, kReacqWaves = kReacqBlock / 64;
struct ReacquireArgs {
    const klt_feat *list;               // Lk
    const klt_ident *prev;              // I(k-1) (null in a begin)
    klt_ident *ident;                   // Ik
    const klt_descriptor *p, *q;        // P, Q
    klt_bank_entry *bank;
    int *state;
    klt_descriptor *fresh_desc;
    int *fresh_slot;
    int4 *bank_best, *fresh_best;
    int n, k, capacity, max_gap;
    klt_match_params mp;                // (cross_check is not read: always on)
};

struct AffineArgs {
    const klt_feat *in;      // records before the translation tracker (frame-1 positions)
    klt_feat *out;           // records after it (updated in place)
    klt_affine_rec *rec;     // per-feature state
    float *tpl;              // [n][3][(height+2)*(width+2)] templates: image, gradx, grady
    const float *i1, *gx1, *gy1, *i2, *gx2, *gy2;     // level 0 of the two frames
    int n, ncols, nrows, mode, width, height, max_iterations;
    float step, small, th, th_aff, max_residue, max_differ;
};

struct SelectArgs {
    const float *sat;        // 3 planes (gxx, gxy, gyy), each ncols*nrows
    float *valmap;           // [ny][nx]
    unsigned long long *keys;
    const uint8_t *seedmap;  // may be null; a pixel is blocked when it holds seed_stamp (a live feature's square, or a selection mask's zero)
    uint8_t seed_stamp;
    const float *val_in;     // test hook: eigenvalues given instead of computed (may be null)
    unsigned *hist, *ticket, *info;   // eigen_hist_kernel: 8192 bins, workgroup ticket, threshold info (hist may be null)
    unsigned hist_target;
    const int *hist_slots;            // optional (device): number of free slots; the cut keeps max(hist_target, hist_per_slot * *hist_slots) keys
    unsigned hist_per_slot;           // (both in units of the sampled histogram: every 4th workgroup counts)
    double min_eig;
    int ncols, nrows, bx, by, step, nx, ny, hw, hh, npow2;
};

struct NmsArgs {
    const unsigned long long *keys;
    klt_feat *fl;
    uint32_t *grid_global;   // used when the cell grid does not fit in LDS
    int *placed_out;         // [0] features placed, [1] 1 if the candidates ran out before the list was full
    int *slots;              // scratch [nfeat]: fillable slot indices (REPLACING_SOME)
    klt_affine_rec *aff_rec; // optional: affine state reset for every slot filled (selectGoodFeatures.py:120-128)
    unsigned cell_magic;     // klt_div_magic(cell) (unused when cell == 1)
    int nkeys, nfeat, overwrite_all, d /* mindist-1 */, cell, gw, gh, grid_in_lds;
};

// per-cell quota of the selector (klt_set_select_grid): the cell of pixel (x, y) is (y / ch) * gw + x / cw.  An argument of the quota
// kernels only: the walk under a quota takes NmsArgs followed by it (select_kernels.hip), the walk without one NmsArgs alone.
struct QuotaArgs {
    unsigned *live;          // [gw * gh] features each cell holds: the list's live records, plus (the walk) the features placed so far
    int cw, ch, gw, q;       // cell size in pixels, cells per row, max_per_cell
    int cells;               // gw * gh
    unsigned cw_magic, ch_magic;      // klt_div_magic of cw / ch; 0 for a cell of 65536 pixels or more (every coordinate is in cell 0), unused for 1
};

// parallel minimum-distance passes (select_kernels.hip)
struct MisArgs {
    const unsigned long long *keys;   // [ny*nx] candidate keys of the eigenvalue pass (0 = no candidate)
    uint32_t *st;                     // [ny*nx] state per candidate cell
    uint32_t *list;                   // [tiles * 1024] undecided cells of every 32x32 tile
    unsigned *cnt;                    // [tiles] length of each tile's list
    unsigned *remaining;              // [rounds] undecided candidates left after pass r
    unsigned long long *acc_keys;     // [tiles * acc_cap] accepted candidates of every tile
    unsigned *acc_cnt;                // [tiles] how many of them
    int acc_cap;
    const unsigned *info;             // info[0] = lowest key bin that takes part (top-K prefilter)
    unsigned *cut_dropped;            // set to 1 by mis_init when that bin keeps a valid key out of the passes (info[3]: the histogram is a sample)
    int nx, ny, R /* exclusion radius in cells */, stage /* 1: stage tile + halo in LDS */;
    int bx, by, step;                 // pixel position of cell (i, j) = (bx + i * step, by + j * step)
    const uint8_t *seed;              // optional: [nrows][ncols] squares of the live features and the selection mask's zeros (pixels holding seed_stamp); keys were scored WITHOUT it
    uint8_t seed_stamp;               // (klt_select_prepare_async)
    int ncols;
    int sparse;                       // 1: few candidates per tile are expected (a replacement behind the cut): later passes take several tiles per workgroup
};

// ---- timing by the dispatch's own timestamps --------------------------------------------------------------------------------
// klt_timing_enable(ctx, 2): the level-0 launch is enqueued with hipExtLaunchKernelGGL and a start / stop event pair that the runtime
// fills from the dispatch packet's begin and end timestamps -- the duration rocprofv3 reports for the kernel.  An event pair recorded
// around a launch (mode 1) also holds the boundary between two dependent launches (~2.6 us).  The API sets the two events, the next
// launch that goes through klt_launch takes them.
extern thread_local hipEvent_t g_klt_stamp_start, g_klt_stamp_stop;

#include <hip/hip_ext.h>
template <typename... Args, typename F = void (*)(Args...)>
inline void klt_launch(F kernel, const dim3 &grid, const dim3 &block, unsigned lds, hipStream_t s, Args... args)
{
    if (g_klt_stamp_start) {
        hipEvent_t a = g_klt_stamp_start, b = g_klt_stamp_stop;
        g_klt_stamp_start = g_klt_stamp_stop = nullptr;
        hipExtLaunchKernelGGL(kernel, grid, block, lds, s, a, b, 0, args...);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    }
}

// ---- launchers (each enqueues on `s`; no synchronisation) ----
void launch_hconv_u8(hipStream_t s, const uint8_t *in, int ncols, int nrows, float *outA, float *outB,
                     int out_cols, int xstride, int xoff, const Taps &ta, const Taps *tb);
void launch_hconv_f32(hipStream_t s, const float *in, int ncols, int nrows, float *outA, float *outB,
                      int out_cols, int xstride, int xoff, const Taps &ta, const Taps *tb);
void launch_take_strided(hipStream_t s, const float *src, float *dst, size_t n, int stride);
void launch_put_strided(hipStream_t s, const float *src, float *dst, size_t n, int stride);     // dst[i * stride] = src[i]
// ostride: element stride of the output plane(s) -- KLT_PIX_STRIDE when outA / outB are planes of a level's pixel records, 1 for
// separate planes (stated by the caller, never inferred from the pointers)
void launch_vconv(hipStream_t s, const float *inA, const float *inB, int ncols, int nrows, float *outA, float *outB,
                  int out_rows, int ystride, int yoff, const Taps &ta, const Taps *tb, int ostride = 1);

// Plane accesses as raw buffer operations (device code): the plane pointer is workgroup-uniform (a descriptor in four
// SGPRs), the lane's 32-bit BYTE offset is the whole vector address.  With `plane + (size_t)y * nc + x` every access costs a
// 64-bit multiply-add (a quarter-rate instruction) and a 64-bit add; 32-bit offsets are a 24-bit multiply (full rate) and 32-bit adds.  (A plane is far below 2 GB; word 3 of the descriptor: data format 32 bits, raw dwords.)
typedef __amdgpu_buffer_rsrc_t plane_rsrc;
__device__ __forceinline__ plane_rsrc plane_of(const void *p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void plane_store(plane_rsrc r, unsigned byte_off, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte_off, 0, 0);
}
__device__ __forceinline__ void plane_store2(plane_rsrc r, unsigned byte_off, float2 v)
{
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 w;
    w.x = __builtin_bit_cast(unsigned, v.x); w.y = __builtin_bit_cast(unsigned, v.y);
    __builtin_amdgcn_raw_buffer_store_b64(w, r, byte_off, 0, 0);
}

__device__ __forceinline__ void plane_store4(plane_rsrc r, unsigned byte_off, float2 a, float2 b)
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 w;
    w.x = __builtin_bit_cast(unsigned, a.x); w.y = __builtin_bit_cast(unsigned, a.y);
    w.z = __builtin_bit_cast(unsigned, b.x); w.w = __builtin_bit_cast(unsigned, b.y);
    __builtin_amdgcn_raw_buffer_store_b128(w, r, byte_off, 0, 0);
}
__device__ __forceinline__ float plane_load(plane_rsrc r, unsigned byte_off)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}

// ---- shared by the level-0 kernels (pyramid_kernels.hip) and the tracker's level-0 gradients on demand (track_kernels.hip): one text, so
// that the two cannot drift apart.  (Both files switch contraction off for the whole translation unit, as the build's flags do.)
// The reflect map for indices at most n beyond either end (frames at least as large as the halo): branch-free
__host__ __device__ __forceinline__ int reflect_once(int i, int n)
{
    return i < 0 ? -1 - i : i >= n ? 2 * n - 1 - i : i;
}

template <int NT>
struct TapRegs { double k[NT]; };

// Register-blocked variant (the one dispatched for the default sigmas).  Every thread produces 4 horizontally
// adjacent samples per step: LDS is read 16 bytes at a time (ds_read_b128, one aligned quad per lane), each
// sample is widened to f64 once per quad instead of once per tap, and the integer index math is amortised over
// four outputs.  The per-output FP64 expression and its operation order are unchanged.
// Column frames (relative to the tile's first output column): A (raw) starts at -8, B / C at -4, D / E at 0,
// all row strides are multiples of 4 floats.  Needs tap radii <= 4.
// ZC (antisymmetric taps only): the centre tap is +0.0 and the centre sample is >= +0 and finite, so the first product c[0] * k[H]
// is +0 and the first addition +0 + p equals p + 0.0 bit for bit (-0 included): the multiply is dropped, the addition kept.
template <int NT, int SYM, bool ZC = false>
__host__ __device__ __forceinline__ float corr_regs(const double *c /* centre */, const TapRegs<NT> &t)
{
    constexpr int H = NT / 2;
    static_assert(!ZC || SYM < 0, "centre-tap elision is for the derivative taps");
    double acc = ZC ? (c[-H] - c[H]) * t.k[0] + 0.0 : c[0] * t.k[H];
#pragma unroll
    for (int jj = ZC ? -H + 1 : -H; jj < 0; jj++) {
        const double pr = SYM > 0 ? c[jj] + c[-jj] : c[jj] - c[-jj];
        acc = acc + pr * t.k[H + jj];
    }
    return (float)acc;
}

extern int g_track_variant;         // KLT_OPT_TRACK_VARIANT (read by the tracker's request builder alone, api_track.hip): 4 (default) quad-load kernels where they apply, 0 always track_kernel
size_t pyr_reduce_lds_bytes(int ss, int ntaps);
// the kernel, form and grid that plan_level0 (l0_plan.h) chose for these arguments: a lean plan writes the smoothed image to the compact
// planes a.cimg and nothing to a.rec, a plan with hred writes the H1 planes a.h1 as well
int launch_smooth_grad(hipStream_t s, const SmoothGradArgs &a, const L0Plan &plan);
int launch_pyr_vreduce(hipStream_t s, const PyrReduceArgs &a, int batch);
int launch_pyr_reduce(hipStream_t s, const PyrReduceArgs &a, int batch);

// Eigenvalue and sort key of one candidate window from its three window sums (goodFeaturesUtils.pyx:17-19 as compiled: (gxx-gyy)^2 in f32,
// 4*gxy*gxy and the sum in f64, pow(., 0.5) -> f32, (gxx+gyy-s) in f32, /2 exact); key 0 = not a candidate (val < max(min_eigenvalue, 1)).
// One definition for every kernel that scores windows (select_kernels.hip, sat_pipeline.hip).
__device__ __forceinline__ float klt_window_value(float gxx, float gxy, float gyy)
{
    const float dif = gxx - gyy;
    const float sq = dif * dif;
    const double t = (double)sq + (4.0 * (double)gxy) * (double)gxy;
    const float s = (float)sqrt(t);
    const float sum = gxx + gyy;
    const float num = sum - s;
    return (float)((double)num / 2.0);
}

// A candidate's key: [f32 bits of val : 32 | x : 16 | y : 16], so that u64 order is (val, x, y) order for val > 0.  The split is
// written here and nowhere else (host and device).
__host__ __device__ __forceinline__ unsigned long long klt_pack_key_bits(uint32_t val_bits, int x, int y)
{
    return ((unsigned long long)val_bits << 32) | ((unsigned long long)x << 16) | (unsigned long long)y;
}
__host__ __device__ __forceinline__ unsigned long long klt_pack_key(float val, int x, int y)
{
    return klt_pack_key_bits(__builtin_bit_cast(uint32_t, val), x, y);
}
__host__ __device__ __forceinline__ int klt_key_x(unsigned long long key) { return (int)((key >> 16) & 0xffffull); }
__host__ __device__ __forceinline__ int klt_key_y(unsigned long long key) { return (int)(key & 0xffffull); }
__host__ __device__ __forceinline__ uint32_t klt_key_bits(unsigned long long key) { return (uint32_t)(key >> 32); }
__host__ __device__ __forceinline__ float klt_key_val(unsigned long long key) { return __builtin_bit_cast(float, klt_key_bits(key)); }

// n / d without an integer division, exact for n < 65536 and 2 <= d < 65536: magic = floor(2^32 / d) + 1 (d == 1 has no magic
// number in 32 bits: callers that allow it test for it)
__host__ __device__ __forceinline__ unsigned klt_div_magic(unsigned d) { return (unsigned)((1ull << 32) / d) + 1u; }
__device__ __forceinline__ unsigned klt_div_by_magic(unsigned n, unsigned magic) { return __umulhi(n, magic); }

// the affine state of a freshly selected feature (selectGoodFeatures.py:120-128)
__host__ __device__ __forceinline__ klt_affine_rec klt_affine_rec_initial()
{
    klt_affine_rec r;
    r.aff_x = -1.f; r.aff_y = -1.f; r.Axx = 1.f; r.Ayx = 0.f; r.Axy = 0.f; r.Ayy = 1.f; r.valid = 0; r.pad = 0;
    return r;
}

__device__ __forceinline__ unsigned long long klt_window_key(float gxx, float gxy, float gyy, double min_eig, int x, int y, float *val_out)
{
    const float val = klt_window_value(gxx, gxy, gyy);
    *val_out = val;
    return (double)val >= min_eig ? klt_pack_key(val, x, y) : 0ull;          // val >= max(min_eigenvalue, 1) > 0
}

// the smallest f32 that is >= m: for an f32 v, (double)v >= m exactly when v >= klt_threshold_f32(m) -- the test without the conversion
// and the f64 compare (a kernel that scores windows waits for its CU's f64 pipes)
inline float klt_threshold_f32(double m)
{
    float t = (float)m;
    if ((double)t < m) t = nextafterf(t, INFINITY);
    return t;
}

void launch_sat_rows(hipStream_t s, const float *gx, const float *gy, float *sat, int ncols, int nrows);
void launch_sat_cols(hipStream_t s, float *sat, int ncols, int nrows);
// step-synchronous wavefront pipelines (sat_pipeline.hip); return 0 or a hipError_t
int  launch_sat_rows_pipe(hipStream_t s, const float *gx, const float *gy, float *sat, int ncols, int nrows);
int  launch_sat_cols_pipe(hipStream_t s, float *sat, int ncols, int nrows);
// column pass + eigenvalue keys in one launch (the column-summed tables never reach HBM); `sat` holds the ROW-summed planes, followed by
// a pad of KLT_SAT_PAD floats (the last strip reads past a row's end), and is only read; keys only (no seed map, value map, histogram or given values); -1 = not applicable (the caller runs the two separate kernels)
constexpr int KLT_SAT_PAD = 64;
bool sat_cols_eigen_ok(const SelectArgs &a);
int  launch_sat_cols_eigen_pipe(hipStream_t s, const float *sat, const SelectArgs &a);
void launch_seed_fill(hipStream_t s, const klt_feat *fl, int nfeat, uint8_t *seedmap, int ncols, int nrows, int d, uint8_t stamp);
// a selection mask of n bytes (16-byte aligned; 0 = never a candidate) merged into the seed map, which has room for n rounded up to 16
void launch_seed_mask(hipStream_t s, const uint8_t *mask, uint8_t *seedmap, size_t n, uint8_t stamp);
void launch_eigen(hipStream_t s, const SelectArgs &a);
void launch_sort_desc(hipStream_t s, unsigned long long *keys, int npow2);
void launch_topk_prefilter(hipStream_t s, const unsigned long long *keys, int n, unsigned target, unsigned *hist,
                           unsigned *info /* [0] bin, [1] kept (histogram), [2] valid, [3] compaction counter */, unsigned long long *out);
int  launch_nms(hipStream_t s, const NmsArgs &a, const QuotaArgs *g);   // the greedy walk, under a quota when g is given; returns 0 or a hipError_t
void launch_key_threshold(hipStream_t s, const unsigned long long *keys, int n, unsigned target, unsigned *hist, unsigned *info);
int  mis_tiles(int nx, int ny);
size_t mis_stage_bytes(int R);
size_t mis_pass_lds(const MisArgs &a);               // dynamic LDS of a pass: the staged tiles + the tile's accepted candidates
void launch_mis_init(hipStream_t s, const MisArgs &a);
int  launch_mis_round(hipStream_t s, const MisArgs &a, int round);   // returns 0 or a hipError_t
void launch_mis_compact(hipStream_t s, const MisArgs &a, unsigned long long *out, unsigned *out_count);
int  mis_tile_capacity(int R);
void launch_zero_words(hipStream_t s, unsigned *p, size_t n);
void launch_mis_prepare(hipStream_t s, const klt_feat *fl, int nfeat, int overwrite_all, int *slots, int *nfill_out, klt_feat *snapshot,
                        unsigned *zero, size_t zero_n);
void launch_eigen_hist(hipStream_t s, const SelectArgs &a);
// histogram (every 4th block of 256 keys, as eigen_hist_kernel samples) of the keys outside the seed map, then the threshold
void launch_mask_hist(hipStream_t s, const SelectArgs &a);
void launch_mis_results(hipStream_t s, unsigned *host_out, const unsigned *rem, int look, const unsigned *info, const int *placed);
// nkept: null, or the keys went through launch_quota_filter (zero keys are skipped, *nkept of them are not zero)
void launch_mis_place(hipStream_t s, const NmsArgs &a, const unsigned *count, const unsigned *nkept, unsigned *rank, const int *nfill, int bound,
                      unsigned *host_out, const unsigned *rem, int look, const unsigned *info);
void launch_unpack_candidates(hipStream_t s, const unsigned long long *keys, int n, float *val, int *x, int *y);
// ---- per-cell quota (klt_set_select_grid)
constexpr int KLT_QUOTA_MAX_ROUNDS = 64;      // largest max_per_cell the filter in front of the rank placement takes (one launch per round)
// g.live[cell] += the list's live records in that cell (g.live zeroed by the caller)
void launch_quota_live(hipStream_t s, const klt_feat *fl, int nfeat, int ncols, int nrows, const QuotaArgs &g);
// keys[0 .. *count) unsorted accepted candidates: those beyond their cell's room become 0, *nkept = how many stay.  thr: 3 planes of `ncells`
// words, zeroed by the caller, like *nkept; g.q <= KLT_QUOTA_MAX_ROUNDS
void launch_quota_filter(hipStream_t s, unsigned long long *keys, const unsigned *count, int bound, const QuotaArgs &g,
                         unsigned long long *thr, int ncells, unsigned *nkept);

void launch_track_stats(hipStream_t s, const klt_feat *in, const klt_feat *out, int n, int nlevels, unsigned long long *stats);
// the kernel, form, grid and LDS that plan_track (track_plan.h) chose for these arguments, behind track_order_kernel where the plan takes a
// feature order and a.order_refresh asks for a new one.  A lazy plan reads level 0 of every pair as a compact image plane (TrackLazyArgs)
// under the gradient taps kg / kd; a gain / bias plan goes to the kernels of track_light_kernels.hip, through the second function
void launch_track(hipStream_t s, const TrackPlan &plan, const TrackGuessArgs &a, const double *kg, const double *kd);
void launch_track_light_kernel(hipStream_t s, const TrackPlan &plan, const TrackArgsBase &a);
// per-feature track quality (quality_kernels.hip): one klt_quality record per feature; returns -1 for an unsupported window
int launch_track_quality(hipStream_t s, const QualityArgs &a);
// the motion-model check (model_kernels.hip), three launches in stream order: candidates, one score per hypothesis, the decision
void launch_model_gather(hipStream_t s, const ModelArgs &a);
void launch_model_score(hipStream_t s, const ModelArgs &a);
void launch_model_decide(hipStream_t s, const ModelArgs &a);
// the epipolar check (epipolar_kernels.hip) behind launch_model_gather: one score per hypothesis, the decision
void launch_epipolar_score(hipStream_t s, const EpipolarArgs &a);
void launch_epipolar_decide(hipStream_t s, const EpipolarArgs &a);
// the homography check (homography_kernels.hip) behind launch_model_gather, likewise
void launch_homography_score(hipStream_t s, const EpipolarArgs &a);
void launch_homography_decide(hipStream_t s, const EpipolarArgs &a);
// the crowding check (crowd_kernels.hip): classify the records and clear the cell counts; every candidate's place in its cell; then one
// workgroup per list groups them by cell, resolves, writes
void launch_crowd_prepare(hipStream_t s, const CrowdArgs &a);
void launch_crowd_rank(hipStream_t s, const CrowdArgs &a);
void launch_crowd_resolve(hipStream_t s, const CrowdArgs &a);
// CLAHE (equalize_kernels.hip): the per-tile LUTs, then the interpolated frame; `batch` frames each
void launch_clahe_lut(hipStream_t s, const EqualizeArgs &a, int batch);
void launch_clahe_apply(hipStream_t s, const EqualizeArgs &a, int batch);
// remap (remap_kernels.hip): the a.batch frames in one launch
void launch_remap(hipStream_t s, const RemapArgs &a);
// descriptors and their matcher (describe_kernels.hip, match_kernels.hip)
void launch_describe(hipStream_t s, const DescribeArgs &a, int mode);
void launch_match(hipStream_t s, const MatchArgs &a);
void launch_match_resolve(hipStream_t s, const MatchResolveArgs &a);
// track identities (reacquire_kernels.hip): the begin launch; a step's classify / deposit / compact launch, its two nearest-neighbour
// launches (bank entries against fresh records: the rule's queries; fresh records against bank entries: the cross-check) and its assign launch
void launch_reacquire_begin(hipStream_t s, const ReacquireArgs &a);
void launch_reacquire_classify(hipStream_t s, const ReacquireArgs &a);
void launch_reacquire_nearest(hipStream_t s, const ReacquireArgs &a, bool of_bank);
void launch_reacquire_assign(hipStream_t s, const ReacquireArgs &a);
void launch_predict_cv(hipStream_t s, const klt_feat *prev, const klt_feat *cur, klt_feat *guess, int n);
void launch_extract_patch(hipStream_t s, const float *img, int nc, int nr, float x, float y, int w, float *patch, int *bad);
void launch_track_iterate(hipStream_t s, const float *t_gx, const float *t_gy, const float *t_i, const float *i2, const float *gx2,
                          const float *gy2, int nc, int nr, int w, float x2, float y2, float step, float small, float th,
                          int max_iterations, float *res);
void launch_affine(hipStream_t s, const AffineArgs &a);
void launch_affine_reset(hipStream_t s, klt_affine_rec *rec, int n);   // returns 0, or -1 for an unsupported window

// ---- multi-GPU (comm.hip): RCCL communicator + side stream; every function returns 0 or a klt_status and fills `err` ----
struct KltComm;
int  comm_unique_id(void *out128, std::string &err);
int  comm_create(int device, int nranks, int rank, const void *unique_id, KltComm **out, std::string &err);
void comm_destroy(KltComm *k);
bool comm_poisoned(const KltComm *k);         // a host-side wait timed out: nothing may wait for this communicator's stream again
int  comm_nranks(const KltComm *k);
hipEvent_t comm_last_done(const KltComm *k);   // end of the most recent collective (an event of the communicator's ring)
int  comm_rank(const KltComm *k);
int  comm_allgather(KltComm *k, hipStream_t producer, const void *src, void *dst, size_t bytes, std::string &err);
int  comm_gather(KltComm *k, hipStream_t producer, const void *src, void *dst, size_t bytes, int root, std::string &err);
int  comm_gatherv(KltComm *k, hipStream_t producer, const void *src, void *dst, const size_t *counts, int root, std::string &err);
void comm_set_timeout(KltComm *k, double ms);
int  comm_sendrecv(KltComm *k, hipStream_t producer, const void *src, int to, void *dst, int from, size_t bytes, std::string &err);
int  comm_fence(KltComm *k, hipStream_t consumer, std::string &err);
int  comm_wait(KltComm *k, std::string &err);
int  comm_allreduce_max(KltComm *k, double *inout, int n, std::string &err);
