// Per-feature coarse-to-fine translational KLT tracker: one wavefront per feature, every pyramid
// level inside one launch (gfx950).
//
// Reference call chain replaced: KLTTrackFeatures per-feature loop (trackFeatures.py:250-346) ->
// _trackFeature (:67-136) -> extractImagePatchSlow (trackFeaturesUtils.pyx:14-51) and
// trackFeatureIterateCKLT (:393-459).  15 000 Python->C calls per 1080p pair become one kernel.
//
// Work split inside the wavefront (window w x w, n = w*w samples):
//   * lane l owns window samples l, l+64, ...; it keeps the image-1 template (intensity, gx, gy) of
//     those samples in registers for the whole level and re-samples image 2 each Newton iteration;
//   * every lane forms the five product terms of its samples (gx*gx, gx*gy, gy*gy, diff*gx, diff*gy) and
//     writes them to LDS; lanes 0..4 then add one array each in the reference's row-major sequential f32
//     order (trackFeaturesUtils.pyx:263-267, :296-302) and the five sums are broadcast with wave
//     shuffles; every lane solves the 2x2 system redundantly so the position stays wave-uniform;
//   * the residue test reproduces numpy's pairwise f32 sum (trackFeatures.py:124).
// The arithmetic mirrors the compiled reference exactly: bilinear weights in FP64
// except the ax*ay*I term which the reference evaluates in f32, products and sums un-fused, f32
// position updates, the in-loop bounds test with the integer half-window and the post-loop one with
// the Python-3 float half-window.
#include <cstdlib>
#include <type_traits>

#include "klt_internal.h"
#include "track_primitives.h"

#pragma clang fp contract(off)

// tools/track_clocks.py builds this file with KLT_TRACK_CLOCKS into a private copy of the library: lane 0 of the first 256
// features of a launch records wall-clock ticks at the marks below (every mark first waits for all outstanding memory
// operations, so the build is for reading the time line, not for timing the kernel).
#ifdef KLT_TRACK_CLOCKS
__device__ long long g_tclk[256 * 32];
#define TCLK(i)                                                                                               \
    do {                                                                                                      \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                            \
        if (threadIdx.x == 0 && blockIdx.x < 256 && (i) < 32) g_tclk[blockIdx.x * 32 + (i)] = wall_clock64();   \
    } while (0)
extern "C" int klt_debug_track_clocks(long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tclk), sizeof(g_tclk)); }
#else
#define TCLK(i) do { } while (0)
#endif

namespace {

// (tried as shared functions and not kept -- each moved register figures of instantiations it was inlined into, in every form tried
// (by value / by reference, one expression / early returns / bitwise, with and without branch hints), so these statements stay
// written out where they are used; tools/kernel_regs.py figures, vgpr / sgpr / scratch:
//   the in-loop bounds test (:428-431): track_kernel<1,0,false,false> 61/73 -> 63/74, track_kernel_quad<false,7,1,false,false>
//       120/68 -> 116/70, <false,15,5,false,false> scratch 40 -> 44, track_iterate_kernel 49/64 -> 50/62;
//   the template footprint test (:35): track_kernel<1,0,true,false> 61/83 -> 63/81, extract_patch_kernel 40 -> 38 VGPRs;
//   the post-loop bounds test (trackFeatures.py:110) and the level status (:127-129): neutral in track_level, but
//       track_kernel_quad<false,7,1,false,false> 68 -> 64 SGPRs resp. <false,7,1,true,false> 68 -> 66, which leaves one caller;
//   the kernels' prologue (feature index, per-pair pointers): track_kernel<1,0,false,false> 61/73 -> 59/77,
//       track_kernel_quad<false,7,1,true,false> 68 -> 66 SGPRs;
//   the run-time-n sum loop shared by track_level and track_iterate_kernel: track_kernel<1,0,false,false> 73 -> 72 SGPRs.
// The primitives now in track_primitives.h moved there with identical assembly; the statements listed here did not, and must not be moved
// the same way without the same comparison.)

// the level with the two frames in each other's place
__device__ __forceinline__ TrackLevel exchanged(const TrackLevel &l)
{
    TrackLevel e;
    e.i1 = l.i2; e.gx1 = l.gx2; e.gy1 = l.gy2;
    e.i2 = l.i1; e.gx2 = l.gx1; e.gy2 = l.gy1;
    e.nc = l.nc; e.nr = l.nr;
    return e;
}

// _trackFeature for one level.  Returns the status; x2/y2 updated in place; `iters` = Newton iterations.
// WCT > 0: window size known at compile time (index math folds, the summation loops unroll and read LDS
// 16 bytes at a time); WCT == 0: any odd window up to 31.
template <int MAXK, int WCT>
__device__ int track_level(const TrackArgsBase &a, const TrackLevel &lv, float x1, float y1, float &x2r, float &y2r,
                           float *lds, int lane, int &iters, int clk0 = 0)
{
    const int w = WCT > 0 ? WCT : a.window, n = w * w, hw = w / 2;
    const int npad = track_npad(n);
    const int nc = lv.nc, nr = lv.nr;
    float *l_diff = lds;                                 // residue scratch (aliases product array 0)
    iters = 0;

    // image-1 template (trackFeatures.py:102-104)
    const Bilinear b1 = make_bilinear(x1, y1);
    if (!(b1.ix - hw >= 0 && b1.iy - hw >= 0 && b1.ix + hw + 2 <= nc && b1.iy + hw + 2 <= nr))
        return KLT_OOB;      // the reference asserts here (trackFeaturesUtils.pyx:35); see DESIGN.md
    float t_i[MAXK], t_gx[MAXK], t_gy[MAXK];
    int off[MAXK];           // sample offset relative to the window's top-left footprint pixel
#pragma unroll
    for (int kk = 0; kk < MAXK; kk++) {
        const int k = lane + 64 * kk;
        t_i[kk] = t_gx[kk] = t_gy[kk] = 0.f;
        off[kk] = 0;
        if (k < n) {
            off[kk] = (k / w) * nc + (k % w);
            const size_t q = (size_t)(b1.iy - hw) * nc + (b1.ix - hw) + off[kk];
            t_i[kk] = sample<KLT_PIX_STRIDE>(lv.i1 + KLT_PIX_STRIDE * q, nc, b1);
            t_gx[kk] = sample<KLT_PIX_STRIDE>(lv.gx1 + KLT_PIX_STRIDE * q, nc, b1);
            t_gy[kk] = sample<KLT_PIX_STRIDE>(lv.gy1 + KLT_PIX_STRIDE * q, nc, b1);
        }
    }

    TCLK(clk0);                                          // template sampled
    float x2 = x2r, y2 = y2r;
    int status;
    const float one_plus_eps = 1.001f;
    for (;;) {
        // trackFeaturesUtils.pyx:428-431 (integer half-window, f32 arithmetic)
        if ((double)(x2 - (float)hw) < 0. || (float)nc - (x2 + (float)hw) < one_plus_eps ||
            (double)(y2 - (float)hw) < 0. || (float)nr - (y2 + (float)hw) < one_plus_eps) {
            status = KLT_OOB;
            break;
        }
        const Bilinear b2 = make_bilinear(x2, y2);
        const size_t base = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
        // every lane forms the five products of its samples (each product is one rounded f32 multiply, exactly the
        // term the reference adds); LDS then holds five arrays of n terms
#pragma unroll
        for (int kk = 0; kk < MAXK; kk++) {
            const int k = lane + 64 * kk;
            if (k < n) {
                const size_t q = base + off[kk];
                const float diff = t_i[kk] - sample<KLT_PIX_STRIDE>(lv.i2 + KLT_PIX_STRIDE * q, nc, b2);          // :82-85
                const float sx = t_gx[kk] + sample<KLT_PIX_STRIDE>(lv.gx2 + KLT_PIX_STRIDE * q, nc, b2);          // -( -g1 - g2 ), :128 and :297
                const float sy = t_gy[kk] + sample<KLT_PIX_STRIDE>(lv.gy2 + KLT_PIX_STRIDE * q, nc, b2);
                lds[k] = sx * sx;                  // gxx terms, :299
                lds[npad + k] = sx * sy;           // gxy terms, :300
                lds[2 * npad + k] = sy * sy;       // gyy terms, :301
                lds[3 * npad + k] = diff * sx;     // ex terms,  :265
                lds[4 * npad + k] = diff * sy;     // ey terms,  :266
            }
        }
        __syncthreads();
        if (iters < 3) TCLK(clk0 + 1 + 2 * iters);       // image 2 sampled, products in LDS
        // lanes 0..4 each add one array in the reference's row-major order (sequential f32 adds)
        float acc = 0.f;
        if (lane < 5) {
            const float *T = lds + lane * npad;
            if constexpr (WCT > 0) acc = chain_sum<WCT * WCT, false, (WCT <= 8 ? 16 : 4)>(reinterpret_cast<const float4 *>(T));
            else
                for (int k = 0; k < n; k++) acc = acc + T[k];
        }
        __syncthreads();
        const float gxx = __shfl(acc, 0), gxy = __shfl(acc, 1), gyy = __shfl(acc, 2);
        const float ex = __shfl(acc, 3) * a.step, ey = __shfl(acc, 4) * a.step;
        float dx, dy;
        if (solve_step(gxx, gxy, gyy, ex, ey, a.small, dx, dy)) { status = KLT_SMALL_DET; break; }
        status = KLT_TRACKED;
        x2 = x2 + dx;
        y2 = y2 + dy;
        if (iters < 3) TCLK(clk0 + 2 + 2 * iters);       // sums, solve, update
        iters++;
        if (!((fabsf(dx) >= a.th || fabsf(dy) >= a.th) && iters < a.max_iterations)) break;
    }
    x2r = x2;
    y2r = y2;
    TCLK(clk0 + 7);                                      // Newton loop left

    // trackFeatures.py:110 -- Python floats: half-window 3.5, eps 1.001 as doubles
    const double x2d = (double)x2, y2d = (double)y2, hwd = a.half_window;
    if (x2d - hwd < 0.0 || (double)nc - (x2d + hwd) < 1.001 || y2d - hwd < 0.0 || (double)nr - (y2d + hwd) < 1.001)
        status = KLT_OOB;

    // residue, trackFeatures.py:118-125
    if (status == KLT_TRACKED && a.use_max_residue) {
        const Bilinear b2 = make_bilinear(x2, y2);
        const size_t base = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
#pragma unroll
        for (int kk = 0; kk < MAXK; kk++) {
            const int k = lane + 64 * kk;
            if (k < n) l_diff[k] = fabsf(t_i[kk] - sample<KLT_PIX_STRIDE>(lv.i2 + KLT_PIX_STRIDE * (base + off[kk]), nc, b2));
        }
        __syncthreads();
        float s = pairwise_sum_wave(l_diff, n, lane);
        __syncthreads();
        s = __shfl(s, 0);
        if (s / (float)n > a.max_residue) status = KLT_LARGE_RESIDUE;
    }
    TCLK(clk0 + 8);                                      // residue test done

    if (a.retain) return KLT_TRACKED;                                   // :127-129
    if (status == KLT_SMALL_DET || status == KLT_OOB || status == KLT_LARGE_RESIDUE) return status;
    if (iters >= a.max_iterations) return KLT_MAX_ITERATIONS;
    return KLT_TRACKED;
}

// Forward-backward rule (klt_gpu.h, klt_track_fb_async) for a feature that the forward pass tracked: `ft` the input record, `fwd` the
// forward record, `back` what the tracker gives for `fwd` with the two frames exchanged.  The round trip's error is formed from the f32
// differences; their squares are exact in FP64 and the sum rounds once (explicit round-to-nearest operations: nothing to contract).
__device__ __forceinline__ klt_feat fb_record(double max_e2, const klt_feat &ft, const klt_feat &fwd, const klt_feat &back)
{
    const float dx = back.x - ft.x, dy = back.y - ft.y;
    const double e2 = __dadd_rn(__dmul_rn((double)dx, (double)dx), __dmul_rn((double)dy, (double)dy));
    if (back.val == KLT_TRACKED && e2 <= max_e2) return fwd;
    klt_feat o;
    o.x = -1.f; o.y = -1.f; o.val = KLT_FB_INCONSISTENT; o.aux = fwd.aux;
    return o;
}

// FB: the forward-backward check in the same launch -- the feature's wavefront descends the pyramids from frame 1 into frame 2 and, if
// that tracked it, once more from there with the two frames exchanged; one `out` record (and one `back` record if asked) per feature.
// GUESS: a motion prior (klt_track_guess_async) -- the search in frame 2 starts at the feature's record in the guess
// list instead of at its own position; the template position, and with FB the way back, are what they are without one.
template <bool FB, bool GUESS = false>
using TrackKernArgs = std::conditional_t<GUESS, TrackGuessArgs, std::conditional_t<FB, TrackArgs, TrackArgsBase>>;

// Whether a guess record counts: val >= 0 and both coordinates finite, decided on the bits BEFORE anything is computed from the position
// (a NaN passes every `<` of the bounds tests, and an address would be formed from it)
__device__ __forceinline__ bool guess_counts(const klt_feat &gs)
{
    const uint32_t bx = __float_as_uint(gs.x), by = __float_as_uint(gs.y);
    return gs.val >= 0 && (bx & 0x7f800000u) != 0x7f800000u && (by & 0x7f800000u) != 0x7f800000u;
}

template <int MAXK, int WCT, bool BATCH, bool FB = false, bool GUESS = false>
__global__ __launch_bounds__(64) void track_kernel(TrackKernArgs<FB, GUESS> a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int f = blockIdx.x;
    if (a.order) {
        // XCD-aware order: workgroup (x, y) runs on XCD x % 8 (gridDim.x is a multiple of 8); XCD c takes the c-th eighth of the
        // features sorted by row, so that the eight L2s each see one band of the pyramids instead of all of every plane
        const uint32_t *ord = a.order + (BATCH ? (size_t)blockIdx.y * a.n : (size_t)0);
        const int c = blockIdx.x & 7, j = blockIdx.x >> 3, pos = c * a.order_chunk + j;
        if (j >= a.order_chunk || pos >= a.n) return;
        f = (int)ord[pos];
    }
    const int lane = threadIdx.x;
    if (f >= a.n) return;
    const TrackLevel *levels = BATCH ? a.pairs[blockIdx.y].lv : a.lv;
    const klt_feat *fin = BATCH ? a.pairs[blockIdx.y].in : a.in;
    klt_feat *fout = BATCH ? a.pairs[blockIdx.y].out : a.out;
    klt_feat *fback = nullptr;
    if constexpr (FB) fback = BATCH ? a.pairs[blockIdx.y].back : a.back;
    const klt_feat ft = fin[f];
    if (ft.val < 0) {                       // only live features are tracked, trackFeatures.py:253
        if (lane == 0) {
            fout[f] = ft;
            if (FB && fback) fback[f] = ft;
        }
        return;
    }
    const int L = a.nlevels;
    TCLK(0);
    float xstart = ft.x, ystart = ft.y;     // FB, second pass: the forward result
    klt_feat fwd = ft;
    float xguess = ft.x, yguess = ft.y;     // GUESS: where the forward search starts (without a guess that counts: at the feature itself)
    if constexpr (GUESS) {
        const klt_feat *fguess = BATCH ? a.pairs[blockIdx.y].guess : a.guess;
        if (fguess) {
            const klt_feat gs = fguess[f];
            if (guess_counts(gs)) { xguess = gs.x; yguess = gs.y; }
        }
    }
    // (a do-while whose condition is constant false without FB: the plain kernels are compiled with no loop here at all -- as a counted
    // loop of one round it moved their register figures)
    int pass = 0;
    do {
        // trackFeatures.py:255-265: position at the coarsest resolution (divisions by a power of two: exact)
        float xloc = xstart, yloc = ystart;
        for (int r = 0; r < L; r++) { xloc = xloc * a.inv_ss; yloc = yloc * a.inv_ss; }   // power of two: exact
        float xout = xloc, yout = yloc;
        if constexpr (GUESS) {
            if (pass == 0) {                // the guess at the coarsest resolution, by the same exact divisions
                xout = xguess; yout = yguess;
                for (int r = 0; r < L; r++) { xout = xout * a.inv_ss; yout = yout * a.inv_ss; }
            }
        }
        int val = KLT_TRACKED;
        uint32_t aux = 0;       // 4 bits per level: 0 = level not visited, v = v-1 Newton iterations (saturating at 14)
        for (int r = L - 1; r >= 0; r--) {
            xloc = xloc * a.ss; yloc = yloc * a.ss; xout = xout * a.ss; yout = yout * a.ss;
            int it = 0;
            const TrackLevel lvf = BATCH ? load_level(levels + r) : levels[r];
            const TrackLevel lv = FB && pass ? exchanged(lvf) : lvf;       // backward: frame 2 holds the template, frame 1 is searched
            val = track_level<MAXK, WCT>(a, lv, xloc, yloc, xout, yout, lds, lane, it, 1 + 9 * (L - 1 - r));
            aux |= (uint32_t)(it < 14 ? it + 1 : 15) << (4 * r);      // visited level r with `it` Newton iterations
            if (val == KLT_SMALL_DET || val == KLT_OOB) break;             // :284-285
        }
        if constexpr (!FB) {
            if (lane == 0) fout[f] = track_record(a, val, xout, yout, aux);
        } else {
            const klt_feat o = track_record(a, val, xout, yout, aux);      // wavefront-uniform
            if (pass == 0) {
                fwd = o;
                if (o.val != KLT_TRACKED) {                                // lost on the way forward: the plain tracker's record, both ways
                    if (lane == 0) {
                        fout[f] = o;
                        if (fback) fback[f] = o;
                    }
                    return;
                }
                xstart = o.x; ystart = o.y;
            } else if (lane == 0) {
                fout[f] = fb_record(a.fb_max_e2, ft, fwd, o);
                if (fback) fback[f] = o;
            }
        }
    } while (FB && ++pass < 2);
}

// ------------------------------------------------------------------------------------------------------
// Quad-load tracker kernels.  The (w+1) x (w+1) footprint of a window is loaded as QUADS of four pixels, one 16-byte load per
// lane and image:
//   7x7   the 8x8 footprint is 16 quads -> a feature owns 16 lanes and a wavefront tracks FOUR features in lock step under
//         per-feature predicates (a finished feature keeps its state and idles);
//   15x15 the 16x16 footprint is exactly 64 quads -> one feature per wavefront.
// Lane (row r, quad h) of a feature loads the records of pixels (r, 4h .. 4h + 3) -- 48 contiguous bytes, three 16-byte loads -- and
// computes the window samples (r, 4h .. 4h + 3) from its own quad, the quad below (lane + quads-per-row) and the first pixels of the
// quads to the right (lane + 1, lane + quads-per-row + 1): 3 vector loads per footprint and wavefront, where the one-sample-per-lane
// kernel issues 12 (7x7) or 48 (15x15).  A footprint row is one contiguous run of (w + 1) records.  The bounds test
// and the footprint of the NEXT Newton iteration are issued as soon as the position is known -- for the first iteration of a
// level together with the template's loads -- so a level costs one memory round trip per iteration instead of one more.
// Every feature's arithmetic is track_level's, operation for operation: same bilinear expression, the five product arrays in
// LDS added by lanes 0..4 of the feature in the reference's row-major sequential f32 order, numpy's pairwise sum for the residue.

// KLT_OPT_TRACK_TREE_SUMS: the sum of one value per lane over the LPF lanes of a feature, by a butterfly in registers -- within a
// row of 16 lanes four v_add_f32 with DPP operands (quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror: after each step
// the lanes that were combined hold the same partial sum, so mirroring pairs what xor would pair), across rows ds_bpermute.  Every
// lane ends up with the total.  Same precision as the sequential f32 chain, other ORDER of the additions: not the reference's bits.
template <int LPF>
__device__ __forceinline__ float group_tree_sum(float v)
{
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    if (LPF > 16) v = v + __shfl_xor(v, 16);
    if (LPF > 32) v = v + __shfl_xor(v, 32);
    return v;
}

// ------------------------------------------------------------------------------------------------------
// LAZY (7x7, plain kernels): level 0 of a frame is its compact smoothed image alone (a lean level-0 build, pyramid_kernels.hip), and the
// 16 lanes of a feature make the three record quads of a footprint themselves.  The gradients of an 8 x 8 footprint with corner (cx, cy)
// need the 14 x 14 image patch around it, rows and columns through the reflect map (scipy reflects the smoothed image when it
// differentiates it): horizontal pass of both filters at 14 rows x 8 columns (derivative taps -> D, Gaussian taps -> E), f32 rounding,
// vertical pass at the 8 x 8 footprint (Gaussian taps down D = gradx, derivative taps down E = grady) -- the FP64 expression and the
// operation order of the level-0 kernels (corr_regs itself, klt_internal.h) without the centre-tap elision, so the values are the
// records' bit for bit.  The rows and columns of the patch go through reflect_once.  With two or more levels a feature whose patch would
// leave the frame has left the image at a coarser level before (at subsampling 4 a level-1 window needs 12 pixels of level 0 to the
// edge, the patch 6), and the features of a wavefront that need nothing are placed at the frame's corner, so in the launches that exist
// today the map is a safety clamp that keeps every lane's addresses inside the plane, not a path a result depends on.
// LDS of a feature during the phase: the patch P (14 rows of 16 floats), then D and E (14 rows of 8); it takes the place of the five
// product arrays, which are dead while it runs.  A feature's region is padded so that two features' lanes fall on different banks.
constexpr int LZ_PW = 16, LZ_ROWS = 14, LZ_P = LZ_ROWS * LZ_PW, LZ_DE = LZ_ROWS * 8, LZ_FLOATS = LZ_P + 2 * LZ_DE + 16;

// The taps of one gradient filter, read from the kernel argument (the TrackLazyArgs at offset 0 of the kernarg segment) where they are
// used: the address goes through an empty asm statement so that the scalar loads are not hoisted and held across the Newton loop
static_assert(sizeof(TrackLazyArgs) == sizeof(TrackArgsBase) + 8 * sizeof(double), "the taps lie right behind the plain kernels' argument");
// (corr_regs reads the taps left of and at the centre, t.k[0 .. 3] of the seven)
__device__ __forceinline__ void lazy_taps(TapRegs<7> &t, bool deriv)
{
    typedef const __attribute__((address_space(4))) char *kptr;
    kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(TrackArgsBase) + (deriv ? 4 * sizeof(double) : 0);
    asm volatile("" : "+s"(p));
#pragma unroll
    for (int i = 0; i < 7; i++) t.k[i] = i < 4 ? ((const __attribute__((address_space(4))) double *)p)[i] : 0.0;
}

// The record quads of lane s = 2 qr + qh (footprint row qr, columns 4 qh .. 4 qh + 3) of the footprint at corner (cx, cy) of `plane`
// (nc x nr, at least 14 x 14), for the features that `need` them; the other features of the wavefront go through the same steps on the
// patch at the frame's corner and keep what they hold.  fl: the feature's LDS region.  Every step keeps few values in registers (the
// kernel around it is close to its register budget): the patch comes in two halves, the vertical pass makes one plane's pixel pair at a time.
__device__ __forceinline__ void lazy_records(const float *plane, int nc, int nr, int cx, int cy, bool need, float *fl, int s,
                                             f32x4 &im, f32x4 &gx, f32x4 &gy)
{
    {
        // the patch: lane s takes column cx - 3 + s of the 14 rows (lanes 14 and 15 repeat column 13)
        const plane_rsrc pl = plane_of(plane);
        const int x0 = need ? cx - 3 : 0, y0 = need ? cy - 3 : 0;
        const unsigned col = (unsigned)reflect_once(x0 + (s < 13 ? s : 13), nc);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            float v[LZ_ROWS / 2];
#pragma unroll
            for (int r = 0; r < LZ_ROWS / 2; r++)
                v[r] = plane_load(pl, 4u * (__umul24((unsigned)reflect_once(y0 + 7 * h + r, nr), (unsigned)nc) + col));
#pragma unroll
            for (int r = 0; r < LZ_ROWS / 2; r++) fl[(7 * h + r) * LZ_PW + s] = v[r];
            wave_lds_sync();
        }
    }
    {
        // horizontal pass: lane s takes footprint column s % 8 of the rows s / 8, s / 8 + 2, ...
        TapRegs<7> kg, kd;
        lazy_taps(kg, false);
        lazy_taps(kd, true);
        const float *p = fl + (s >> 3) * LZ_PW + (s & 7);
        float *d = fl + LZ_P + s;
#pragma unroll 1
        for (int j = 0; j < LZ_ROWS / 2; j++, p += 2 * LZ_PW, d += 16) {
            float dd, ee;
            lazy_row_h<1>(p, kg, kd, &dd, &ee);
            d[0] = dd;
            d[LZ_DE] = ee;
        }
    }
    wave_lds_sync();
    f32x4 oi, ox, oy;
    {
        // vertical pass: the lane's own quad -- Gaussian taps down D (gradx), derivative taps down E (grady)
        const int qr = s >> 1, qh = s & 1;
        const float *d = fl + LZ_P + qr * 8 + 4 * qh;
        float o[8];
#pragma unroll 1
        for (int u = 0; u < 4; u++) {                        // u = 2 plane + half
            TapRegs<7> k;
            lazy_taps(k, u >= 2);
            const float *c = d + (u >> 1) * LZ_DE + 2 * (u & 1);
            float c0[7], c1[7];
#pragma unroll
            for (int j = 0; j < 7; j++) {
                const float2 t = *reinterpret_cast<const float2 *>(c + 8 * j);
                c0[j] = t.x; c1[j] = t.y;
            }
            float a0, a1;
            if (u < 2) { lazy_col_v<1, 1>(c0, k, &a0); lazy_col_v<1, 1>(c1, k, &a1); }
            else { lazy_col_v<-1, 1>(c0, k, &a0); lazy_col_v<-1, 1>(c1, k, &a1); }
            // (o[] by a constant index: the loop is not unrolled, so each slot is set under its own test)
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (u == e) { o[2 * e] = a0; o[2 * e + 1] = a1; }
        }
        ox.x = o[0]; ox.y = o[1]; ox.z = o[2]; ox.w = o[3];
        oy.x = o[4]; oy.y = o[5]; oy.z = o[6]; oy.w = o[7];
        const float *c = fl + (qr + 3) * LZ_PW + 3 + 4 * qh;
        oi.x = c[0]; oi.y = c[1]; oi.z = c[2]; oi.w = c[3];
    }
    wave_lds_sync();
    if (need) { im = oi; gx = ox; gy = oy; }
}

// The fused entry phase of level 0 (KLT_OPT_TRACK_LAZY_FORM 1): the template's quads (corner (cx1, cy1) of plane1, for the features that
// need1 them) and those of the first search footprint (corner (cx2, cy2) of plane2, need2) in ONE phase instead of two lazy_records calls
// in a row -- the two patches depend on nothing of each other, so all 28 patch rows are requested before anything waits, and the wavefront
// pays one memory round trip where the two calls pay four.
//   loads   straight into LDS (buffer_load ... lds, 4 bytes per lane): no destination registers, one wait for both patches.  The
//           destination of such a load is a wave-uniform base + lane x 4, so a patch row is one wave-instruction and lies as
//           [feature][16 lanes]; lane s of a feature brings column s of the patch (14 and 15 repeat column 13) through the reflect map.
//           A row is LZE_STRIDE floats from the next.
//   H pass  one lane per patch row (lanes 14 and 15 of a feature idle), one round per patch: the lane reads its 14 samples once, widens each
//           once and slides the window over the 8 footprint columns (lazy_row_h<8>), then writes 8 D and 8 E values over its own row.
//   image   the 8 x 8 image values of a footprint are the middle of the patch rows 3 .. 10, which the H pass overwrites: the lanes of those
//           rows set them aside ([patch][feature][8][8] behind the patches), and every lane reads its quad from there at the end -- held
//           in registers from before the H pass they took the kernel past 128 VGPRs.
//   V pass  one lane per footprint column of a patch, 8 + 8 lanes for the two patches, one round per filter: the lane reads its column of
//           14 values once, widens each once and slides the window down the 8 footprint rows (lazy_col_v<., 8>) -- 14 conversions per
//           column where a lane per pixel pair makes 14 per pair -- and writes the 8 results over the head of its column; every lane
//           then reads the quads of its own pixels.  Each tap set is read once per pass.
// Row stride 72 floats, a multiple of 4 (16-byte row reads) and 8 mod 32: the 16 lanes of a feature's V pass read 8 + 8 consecutive
// floats 16 banks apart; the H pass's 16-byte row reads meet two rows per bank group (r and r + 8).
// Every output is the corr_regs call of lazy_records on the same seven values in the same order: the same bits.
constexpr int LZE_STRIDE = 72, LZE_PATCH = 2 * LZ_ROWS * LZE_STRIDE, LZE_FLOATS = LZE_PATCH + 2 * 4 * 64;

__device__ __forceinline__ void lazy_records_entry(const float *plane1, const float *plane2, int nc, int nr, int cx1, int cy1, bool need1,
                                                   int cx2, int cy2, bool need2, float *lds, int g, int s,
                                                   f32x4 &t_im, f32x4 &t_gx, f32x4 &t_gy, f32x4 &s_im, f32x4 &s_gx, f32x4 &s_gy)
{
    typedef __attribute__((address_space(3))) float *lds_ptr;
    // (the lane's place through an empty asm statement: the LDS addresses of the phase are made here, from it, not at the head of the
    // kernel and held through every level -- there they cost the kernel a spilled register)
    asm volatile("" : "+v"(s), "+v"(g));
    // reflect_once without a comparison per case (28 rows: as selects under tests the compiler made branches of them): -1 - i for i < 0,
    // then the smaller of a and its mirror image 2 n - 1 - a, which is a itself below n
    auto reflect = [](int i, int n) { const int a = i ^ (i >> 31); return min(a, 2 * n - 1 - a); };
    const int sc = s < 13 ? s : 13;
    // (the destination through an empty asm statement: the 28 row addresses are made where they are used, not once per kernel and held)
    lds_ptr dst = (lds_ptr)lds;
    asm volatile("" : "+s"(dst));
    const int xa = need1 ? cx1 - 3 : 0, ya = need1 ? cy1 - 3 : 0, xb = need2 ? cx2 - 3 : 0, yb = need2 ? cy2 - 3 : 0;
    const plane_rsrc pa = plane_of(plane1), pb = plane_of(plane2);
    if (__all(min(min(xa, ya), min(xb, yb)) >= 0 && max(xa, xb) + LZ_ROWS <= nc && max(ya, yb) + LZ_ROWS <= nr)) {
        // no patch of the wavefront leaves its frame (every launch of two or more levels): row r is r rows below the first, and that
        // distance rides in the load's scalar offset -- no vector instruction per row
        const unsigned oa = 4u * (__umul24((unsigned)ya, (unsigned)nc) + (unsigned)(xa + sc));
        const unsigned ob = 4u * (__umul24((unsigned)yb, (unsigned)nc) + (unsigned)(xb + sc));
#pragma unroll
        for (int r = 0; r < LZ_ROWS; r++) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pa, dst + r * LZE_STRIDE, 4, oa, 4 * r * nc, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pb, dst + (LZ_ROWS + r) * LZE_STRIDE, 4, ob, 4 * r * nc, 0, 0);
        }
    } else {
        const unsigned ca = (unsigned)reflect(xa + sc, nc), cb = (unsigned)reflect(xb + sc, nc);
#pragma unroll
        for (int r = 0; r < LZ_ROWS; r++) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pa, dst + r * LZE_STRIDE, 4,
                                                     4u * (__umul24((unsigned)reflect(ya + r, nr), (unsigned)nc) + ca), 0, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(pb, dst + (LZ_ROWS + r) * LZE_STRIDE, 4,
                                                     4u * (__umul24((unsigned)reflect(yb + r, nr), (unsigned)nc) + cb), 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float *const fb = lds + 16 * g;                          // the feature's 16 floats of every row
    const int qr = s >> 1, qh = s & 1;
    float *const im = lds + LZE_PATCH + 64 * g;              // the feature's 8 x 8 image values, of the template (and + 256: the footprint)
    if (s < LZ_ROWS) {
        float4 *row = reinterpret_cast<float4 *>(fb + s * LZE_STRIDE);
        float4 *keep = reinterpret_cast<float4 *>(im + 8 * (s - 3));
        TapRegs<7> kg, kd;
        lazy_taps(kg, false);
        lazy_taps(kd, true);
        // (both rounds unrolled: as a rolled loop the kernel kept 57 SGPRs spilled to VGPR lanes and read them back in here -- 5 us of the
        // eight-pair launch -- and the single-pair kernel reserved scratch)
#pragma unroll
        for (int p = 0; p < 2; p++, row += LZ_ROWS * LZE_STRIDE / 4, keep += 64) {
            const float4 v0 = row[0], v1 = row[1], v2 = row[2], v3 = row[3];
            const float v[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
            if (s >= 3 && s < 11) { keep[0] = make_float4(v[3], v[4], v[5], v[6]); keep[1] = make_float4(v[7], v[8], v[9], v[10]); }
            float d[8], e[8];
            lazy_row_h<8>(v, kg, kd, d, e);
            row[0] = make_float4(d[0], d[1], d[2], d[3]); row[1] = make_float4(d[4], d[5], d[6], d[7]);
            row[2] = make_float4(e[0], e[1], e[2], e[3]); row[3] = make_float4(e[4], e[5], e[6], e[7]);
        }
    }
    wave_lds_sync();
    {
        // vertical pass: lane s takes footprint column s & 7 of patch s >> 3, first down D with the Gaussian taps (gradx), then down E with
        // the derivative taps (grady): its 14 values read and widened once, the window slid down the 8 footprint rows (lazy_col_v<., 8>).
        // The 8 results go over the first 8 rows of the column they came from, which no lane reads again.
        float *col = fb + (s >> 3) * LZ_ROWS * LZE_STRIDE + (s & 7);
#pragma unroll
        for (int pl = 0; pl < 2; pl++, col += 8) {
            TapRegs<7> k;
            lazy_taps(k, pl);
            float c[LZ_ROWS], out[8];
#pragma unroll
            for (int j = 0; j < LZ_ROWS; j++) c[j] = col[j * LZE_STRIDE];
            if (pl) lazy_col_v<-1, 8>(c, k, out);
            else lazy_col_v<1, 8>(c, k, out);
#pragma unroll
            for (int j = 0; j < 8; j++) col[j * LZE_STRIDE] = out[j];
        }
    }
    wave_lds_sync();
    // every lane's quads: the image values set aside, gradx and grady where the vertical pass left them
    const float *qd = fb + qr * LZE_STRIDE + 4 * qh;
    const f32x4 i1 = *reinterpret_cast<const f32x4 *>(im + 4 * s), i2 = *reinterpret_cast<const f32x4 *>(im + 256 + 4 * s);
    const f32x4 x1 = *reinterpret_cast<const f32x4 *>(qd), y1 = *reinterpret_cast<const f32x4 *>(qd + 8);
    const f32x4 x2 = *reinterpret_cast<const f32x4 *>(qd + LZ_ROWS * LZE_STRIDE), y2 = *reinterpret_cast<const f32x4 *>(qd + LZ_ROWS * LZE_STRIDE + 8);
    wave_lds_sync();
    if (need1) { t_im = i1; t_gx = x1; t_gy = y1; }
    if (need2) { s_im = i2; s_gx = x2; s_gy = y2; }
}

// the image values of pixels q .. q + 3 of a compact plane (the residue at a lazy level 0)
__device__ __forceinline__ f32x4 load_plane_images(const float *plane, unsigned q)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(plane_of(plane), 4u * q, 0, 0));
}

// FB: the forward-backward check in the same launch (see track_kernel).  A lane group whose feature is not tracked back -- not live, or
// lost on the way forward -- idles through the second pass under the predicate that masks a finished feature in the first.
// (WAVES = occupancy target + GUESS_WAVES for the instantiations with a prior: the plain ones are looked up by the head of their names --
// batch flag, window, target, sum form -- which has to stay theirs alone; as a shared body under two kernel names the 15x15 kernel took
// 48 instead of 40 bytes of scratch and four plain instantiations two more SGPRs)
// (LAZY, the instantiations that make their level-0 gradients themselves, carry a mark of their own there for the same reason: WAVES =
// occupancy target + LAZY_WAVES; and + ENTRY_WAVES on top for the ones whose level-0 entry is the fused phase, lazy_records_entry)
constexpr int GUESS_WAVES = 8, LAZY_WAVES = 16, ENTRY_WAVES = 32;

template <bool BATCH, int W, int WAVES = 1, bool TREE = false, bool FB = false, bool GUESS = false>
__global__ __launch_bounds__(64, WAVES >= ENTRY_WAVES ? 4 : WAVES % GUESS_WAVES) void track_kernel_quad(std::conditional_t<(WAVES >= LAZY_WAVES), TrackLazyArgs, TrackKernArgs<FB, GUESS>> a)
{
    constexpr bool LAZY = WAVES >= LAZY_WAVES;
    constexpr bool ENTRY = WAVES >= ENTRY_WAVES;             // LAZY: the template and the first footprint of level 0 in one fused phase
    static_assert(GUESS == (WAVES >= GUESS_WAVES && !LAZY), "instantiations with a prior carry the mark in their occupancy target");
    static_assert(!LAZY || (W == 7 && !TREE && !FB && !GUESS), "level-0 gradients on demand: the plain 7x7 kernels only");
    static_assert(W == 7 || W == 15, "quad kernels exist for 7x7 and 15x15 windows");
    static_assert(!(FB && TREE), "the forward-backward check uses the reference-order sums");
    constexpr int FPW = W == 7 ? 4 : 1;                      // features per wavefront
    constexpr int LPF = 64 / FPW;                            // lanes per feature = quads of its footprint
    constexpr int QPR = (W + 1) / 4;                         // quads per footprint row
    constexpr int w = W, n = W * W, hw = W / 2, npad = track_npad(n);
    constexpr bool REUSE = W == 7;                           // keep a footprint whose integer corner has not moved (see request_footprint)
    static_assert((W + 1) * QPR == LPF, "one quad per lane");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, g = lane / LPF, s = lane % LPF, glead = lane - s;
    int f = FPW * blockIdx.x + g;
    if (a.order) {
        // XCD-aware order (KLT_OPT_TRACK_XCD_ORDER): workgroups go to the XCDs round-robin in linear order and gridDim.x is a
        // multiple of 8, so workgroup (x, y) runs on XCD x % 8; it takes FPW consecutive features of that XCD's band of the
        // row-sorted list of its pair (batched launches: pair blockIdx.y, permutation blockIdx.y of the table)
        const uint32_t *ord = a.order + (BATCH ? (size_t)blockIdx.y * a.n : (size_t)0);
        const int c = blockIdx.x & 7, j = FPW * (blockIdx.x >> 3) + g, pos = c * a.order_chunk + j;
        f = (j < a.order_chunk && pos < a.n) ? (int)ord[pos] : a.n;
    }
    const TrackLevel *levels = BATCH ? a.pairs[blockIdx.y].lv : a.lv;
    const klt_feat *fin = BATCH ? a.pairs[blockIdx.y].in : a.in;
    klt_feat *fout = BATCH ? a.pairs[blockIdx.y].out : a.out;
    klt_feat *fback = nullptr;
    if constexpr (FB) fback = BATCH ? a.pairs[blockIdx.y].back : a.back;
    const bool valid = f < a.n;
    const klt_feat ft = fin[valid ? f : a.n - 1];
    const bool tracked_feature = valid && ft.val >= 0;       // only live features are tracked, trackFeatures.py:253
    float xguess = ft.x, yguess = ft.y;                      // GUESS: where the feature's forward search starts (see track_kernel)
    if constexpr (GUESS) {
        const klt_feat *fguess = BATCH ? a.pairs[blockIdx.y].guess : a.guess;
        if (fguess) {
            const klt_feat gs = fguess[valid ? f : a.n - 1];
            if (guess_counts(gs)) { xguess = gs.x; yguess = gs.y; }
        }
    }
    if (valid && ft.val < 0 && s == 0) {
        fout[f] = ft;
        if (FB && fback) fback[f] = ft;
    }
    if (!__any(tracked_feature)) return;
    const int L = a.nlevels;
    float *const gl = lds + g * 5 * npad;                    // this feature's five product arrays
    const int qr = s / QPR, qh = s % QPR;                    // my quad: footprint row qr, columns 4 qh .. 4 qh + 3
    const int k0 = qr * w + 4 * qh;                          // window index of my first sample (qr, 4 qh)
    const float one_plus_eps = 1.001f;

    bool go = tracked_feature;                               // the feature takes part in the pass
    float xstart = ft.x, ystart = ft.y;                      // FB, second pass: the forward result
    klt_feat fwd = ft, bwd = ft;
    // (a do-while whose condition is constant false without FB: the plain kernels are compiled with no loop here at all -- as a counted
    // loop of one round it moved their register figures)
    int pass = 0;
    do {
        // trackFeatures.py:255-265
        float xloc = xstart, yloc = ystart;
        for (int r = 0; r < L; r++) { xloc = xloc * a.inv_ss; yloc = yloc * a.inv_ss; }
        float xout = xloc, yout = yloc;
        if constexpr (GUESS) {
            if (pass == 0) {
                xout = xguess; yout = yguess;
                for (int r = 0; r < L; r++) { xout = xout * a.inv_ss; yout = yout * a.inv_ss; }
            }
        }
        int val = KLT_TRACKED;
        uint32_t aux = 0;
        bool alive = go;                                         // still descending the pyramid

        for (int r = L - 1; r >= 0; r--) {
            if (!__any(alive)) break;
            const TrackLevel lvf = BATCH ? load_level(levels + r) : levels[r];
            const TrackLevel lv = FB && pass ? exchanged(lvf) : lvf;       // backward: frame 2 holds the template, frame 1 is searched
            const int nc = lv.nc, nr = lv.nr;
            if (alive) { xloc = xloc * a.ss; yloc = yloc * a.ss; xout = xout * a.ss; yout = yout * a.ss; }

            // image-1 template (trackFeatures.py:102-104); a window that leaves image 1 ends the feature
            const Bilinear b1 = make_bilinear(xloc, yloc);
            const bool t_ok = b1.ix - hw >= 0 && b1.iy - hw >= 0 && b1.ix + hw + 2 <= nc && b1.iy + hw + 2 <= nr;
            const bool run = alive && t_ok;
            // (row * nc as a 24-bit multiply: both are far below 2^24, and the 32-bit integer multiply is a quarter-rate instruction)
            const unsigned q1 = run ? __umul24((unsigned)(b1.iy - hw + qr), (unsigned)nc) + (unsigned)(b1.ix - hw + 4 * qh) : 0u;   // 32-bit element offsets: scalar base + vector offset loads
            f32x4 t_qi, t_qgx, t_qgy;
            float *const fl = lds + g * LZ_FLOATS;               // LAZY: this feature's patch and gradient intermediates
            if constexpr (LAZY) {
                if (r == 0) {
                    t_qi = f32x4{0.f, 0.f, 0.f, 0.f}; t_qgx = t_qi; t_qgy = t_qi;
                    // (ENTRY: the first request_footprint below makes the template's quads together with the footprint's)
                    if constexpr (!ENTRY) lazy_records(lv.i1, nc, nr, b1.ix - hw, b1.iy - hw, run, fl, s, t_qi, t_qgx, t_qgy);
                } else {
                    load_records(lv.i1, q1, t_qi, t_qgx, t_qgy);
                }
            } else {
                load_records(lv.i1, q1, t_qi, t_qgx, t_qgy);
            }

            // the first Newton iteration starts from a position that is already known: its bounds test (trackFeaturesUtils.pyx:428-431)
            // and its footprint loads go out now, behind the template's
            int it = 0, status = KLT_OOB;
            float x2 = xout, y2 = yout;
            bool iterating = run;
            Bilinear b2;
            f32x4 s_qi = {0.f, 0.f, 0.f, 0.f}, s_qgx = s_qi, s_qgy = s_qi;
            unsigned q_held = ~0u;                               // element offset of the footprint quads in s_q*: none of this level yet
            // A Newton step usually moves the window by less than a pixel: when its integer corner stays where it was, the footprint is
            // the one already in registers (only the bilinear weights change) and nothing is requested; neither is anything for a
            // feature that has stopped.  The launch is bound by the L1's requests to the L2 in flight (tools/pmc_mem.sh: ~78 per CU
            // all the time at ~750 clocks each), so a request not made is time saved: 89.2 -> 86.6 us per eight-pair launch of cfg-2,
            // 131.6 -> 125.7 us at cfg-4.  7x7 only: the 15x15 kernel, at its occupancy target of five, pays for the held offset and the
            // conditional loads with 16 more bytes of scratch and goes from 38.9 to 42.4 us at cfg-3.
            // (first: the request at the level's entry, a type that says so)
            auto request_footprint = [&](auto first) {
                const bool oob = (double)(x2 - (float)hw) < 0. || (float)nc - (x2 + (float)hw) < one_plus_eps ||
                                 (double)(y2 - (float)hw) < 0. || (float)nr - (y2 + (float)hw) < one_plus_eps;
                if (iterating && oob) { status = KLT_OOB; iterating = false; }
                b2 = make_bilinear(x2, y2);
                if (REUSE) {
                    const unsigned q = __umul24((unsigned)(b2.iy - hw + qr), (unsigned)nc) + (unsigned)(b2.ix - hw + 4 * qh);
                    if constexpr (LAZY) {
                        if (r == 0) {
                            const bool need = iterating && q != q_held;
                            if constexpr (ENTRY && decltype(first)::value) {
                                lazy_records_entry(lv.i1, lv.i2, nc, nr, b1.ix - hw, b1.iy - hw, run, b2.ix - hw, b2.iy - hw, need, lds, g, s,
                                                   t_qi, t_qgx, t_qgy, s_qi, s_qgx, s_qgy);
                                // (the weights made again behind the phase, from a position the compiler takes for another: only the
                                // corner is held through it, six registers fewer)
                                float xa = x2;
                                asm volatile("" : "+v"(xa));
                                b2 = make_bilinear(xa, y2);
                            } else if (__any(need)) lazy_records(lv.i2, nc, nr, b2.ix - hw, b2.iy - hw, need, fl, s, s_qi, s_qgx, s_qgy);
                            if (need) q_held = q;
                        } else if (iterating && q != q_held) {
                            load_records(lv.i2, q, s_qi, s_qgx, s_qgy);
                            q_held = q;
                        }
                    } else
                    if (iterating && q != q_held) {
                        load_records(lv.i2, q, s_qi, s_qgx, s_qgy);
                        q_held = q;
                    }
                } else {
                    const unsigned q = iterating ? __umul24((unsigned)(b2.iy - hw + qr), (unsigned)nc) + (unsigned)(b2.ix - hw + 4 * qh) : 0u;
                    load_records(lv.i2, q, s_qi, s_qgx, s_qgy);
                }
            };
            request_footprint(std::true_type{});

            float t_i[4], t_gx[4], t_gy[4];
            sample_quad<QPR>(t_qi, b1, t_i);
            sample_quad<QPR>(t_qgx, b1, t_gx);
            sample_quad<QPR>(t_qgy, b1, t_gy);

            while (__any(iterating)) {
                const bool act = iterating;
                float s_i[4], s_gx[4], s_gy[4];
                sample_quad<QPR>(s_qi, b2, s_i);
                sample_quad<QPR>(s_qgx, b2, s_gx);
                sample_quad<QPR>(s_qgy, b2, s_gy);
                float tree[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // TREE: this lane's share of the five sums (its samples inside the window)
    #pragma unroll
                for (int m = 0; m < 4; m++) {
                    if (qr < w && 4 * qh + m < w) {
                        const int k = k0 + m;
                        const float diff = t_i[m] - s_i[m];
                        const float sx = t_gx[m] + s_gx[m];
                        const float sy = t_gy[m] + s_gy[m];
                        if (TREE) {
                            tree[0] = tree[0] + sx * sx;
                            tree[1] = tree[1] + sx * sy;
                            tree[2] = tree[2] + sy * sy;
                            tree[3] = tree[3] + diff * sx;
                            tree[4] = tree[4] + diff * sy;
                        } else {
                            gl[k] = sx * sx;
                            gl[npad + k] = sx * sy;
                            gl[2 * npad + k] = sy * sy;
                            gl[3 * npad + k] = diff * sx;
                            gl[4 * npad + k] = diff * sy;
                        }
                    }
                }
                if (!TREE) wave_lds_sync();
                float acc = 0.f;
                if (!TREE && s < 5) acc = chain_sum<n, (W > 8), (W > 8 ? 8 : 16)>(reinterpret_cast<const float4 *>(gl + s * npad));
                if (!TREE) wave_lds_sync();
                float gxx, gxy, gyy, ex, ey;
                if (TREE) {
                    gxx = group_tree_sum<LPF>(tree[0]); gxy = group_tree_sum<LPF>(tree[1]); gyy = group_tree_sum<LPF>(tree[2]);
                    ex = group_tree_sum<LPF>(tree[3]) * a.step; ey = group_tree_sum<LPF>(tree[4]) * a.step;
                } else {
                    gxx = __shfl(acc, glead); gxy = __shfl(acc, glead + 1); gyy = __shfl(acc, glead + 2);
                    ex = __shfl(acc, glead + 3) * a.step; ey = __shfl(acc, glead + 4) * a.step;
                }
                float dx, dy;
                const bool small_det = solve_step(gxx, gxy, gyy, ex, ey, a.small, dx, dy);
                if (act && small_det) { status = KLT_SMALL_DET; iterating = false; }
                if (act && !small_det) {
                    status = KLT_TRACKED;
                    x2 = x2 + dx;
                    y2 = y2 + dy;
                    it++;
                    iterating = (fabsf(dx) >= a.th || fabsf(dy) >= a.th) && it < a.max_iterations;
                }
                if (__any(iterating)) request_footprint(std::false_type{});
            }
            if (run) { xout = x2; yout = y2; }

            // trackFeatures.py:110 -- Python floats: half-window 3.5, eps 1.001 as doubles
            const double x2d = (double)x2, y2d = (double)y2, hwd = a.half_window;
            if (run && (x2d - hwd < 0.0 || (double)nc - (x2d + hwd) < 1.001 || y2d - hwd < 0.0 || (double)nr - (y2d + hwd) < 1.001))
                status = KLT_OOB;

            // residue, trackFeatures.py:118-125
            const bool need_res = run && status == KLT_TRACKED && a.use_max_residue;
            if (__any(need_res)) {
                const Bilinear br = make_bilinear(x2, y2);
                f32x4 r_qi;
                if (REUSE) {
                    const unsigned q = __umul24((unsigned)(br.iy - hw + qr), (unsigned)nc) + (unsigned)(br.ix - hw + 4 * qh);
                    r_qi = s_qi;                                 // the last footprint, if the final position has the same integer corner
                    if constexpr (LAZY) {
                        if (need_res && q != q_held) r_qi = r == 0 ? load_plane_images(lv.i2, q) : load_record_images(lv.i2, q);
                    } else
                    if (need_res && q != q_held) r_qi = load_record_images(lv.i2, q);
                } else {
                    const unsigned q = need_res ? __umul24((unsigned)(br.iy - hw + qr), (unsigned)nc) + (unsigned)(br.ix - hw + 4 * qh) : 0u;
                    r_qi = load_record_images(lv.i2, q);
                }
                float s_i[4];
                sample_quad<QPR>(r_qi, br, s_i);
                float sres;
                if (TREE) {
                    float part = 0.f;
    #pragma unroll
                    for (int m = 0; m < 4; m++)
                        if (qr < w && 4 * qh + m < w) part = part + fabsf(t_i[m] - s_i[m]);
                    sres = group_tree_sum<LPF>(part);
                } else {
    #pragma unroll
                    for (int m = 0; m < 4; m++)
                        if (qr < w && 4 * qh + m < w) gl[k0 + m] = fabsf(t_i[m] - s_i[m]);
                    wave_lds_sync();
                    sres = pairwise_sum<3>(gl, n, s);
                    wave_lds_sync();
                    sres = __shfl(sres, glead);
                }
                if (need_res && sres / (float)n > a.max_residue) status = KLT_LARGE_RESIDUE;
            }

            int lvl_val;
            if (!t_ok) lvl_val = KLT_OOB;
            else if (a.retain) lvl_val = KLT_TRACKED;                                               // :127-129
            else if (status == KLT_SMALL_DET || status == KLT_OOB || status == KLT_LARGE_RESIDUE) lvl_val = status;
            else if (it >= a.max_iterations) lvl_val = KLT_MAX_ITERATIONS;
            else lvl_val = KLT_TRACKED;
            if (alive) {
                val = lvl_val;
                aux |= (uint32_t)(it < 14 ? it + 1 : 15) << (4 * r);
                alive = !(val == KLT_SMALL_DET || val == KLT_OOB);                                  // :284-285
            }
        }
        if constexpr (!FB) {
            // (track_record's text, in place: through the function the tree-sum 7x7 instantiations came out two SGPRs apart)
            if (tracked_feature && s == 0) {
                klt_feat o;
                o.aux = (int32_t)aux;
                const double xd = (double)xout, yd = (double)yout;
                const bool oob = val == KLT_OOB ||
                                 xd < a.borderx || xd > (double)(a.ncols - 1) - a.borderx ||
                                 yd < a.bordery || yd > (double)(a.nrows - 1) - a.bordery;   // :288-308
                if (oob) { o.x = -1.f; o.y = -1.f; o.val = KLT_OOB; }
                else if (val == KLT_SMALL_DET || val == KLT_LARGE_RESIDUE || val == KLT_MAX_ITERATIONS) {
                    o.x = -1.f; o.y = -1.f; o.val = val;
                } else { o.x = xout; o.y = yout; o.val = KLT_TRACKED; }
                fout[f] = o;
            }
        } else {
            const klt_feat o = track_record(a, val, xout, yout, aux);          // uniform within the feature's lane group
            if (pass == 0) {
                fwd = o;
                go = go && o.val == KLT_TRACKED;                               // lost on the way forward: the plain tracker's record, both ways
                xstart = o.x; ystart = o.y;
                if (!__any(go)) break;
            } else {
                bwd = o;
            }
        }
    } while (FB && ++pass < 2);
    if constexpr (FB) {
        if (tracked_feature && s == 0) {
            fout[f] = go ? fb_record(a.fb_max_e2, ft, fwd, bwd) : fwd;
            if (fback) fback[f] = go ? bwd : fwd;
        }
    }
}

// (15x15, measured and not kept -- round 2: several features per workgroup with ONE wavefront adding the five 225-term chains of
// all of them (5 NW lanes busy instead of 5; the chains are 40 % of an iteration's instructions): 68.4 us (8 features) / 62.7 (4)
// against 59.8 for one independent wavefront per feature at cfg-3.  The barriers and the lock step cost more than the saved issue
// slots.)

// Features sorted by image row (counting sort, one workgroup): order[0..n) = feature indices by ascending (int)y; lost
// features go last.  The order within a row is whatever the atomics give -- every feature is still tracked exactly once and
// written to its own slot, so the result does not depend on it.
constexpr int ORDER_BINS = 4096, ORDER_T = 1024;
__global__ __launch_bounds__(ORDER_T) void track_order_kernel(const klt_feat *__restrict__ in_single, const TrackPairDesc *__restrict__ pairs,
                                                              int n, uint32_t *__restrict__ order_base)
{
    const klt_feat *__restrict__ in = pairs ? pairs[blockIdx.x].in : in_single;      // batched launches: one workgroup per pair
    uint32_t *__restrict__ order = order_base + (size_t)blockIdx.x * n;
    __shared__ unsigned hist[ORDER_BINS], start[ORDER_BINS];
    __shared__ unsigned wsum[ORDER_T / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < ORDER_BINS; i += ORDER_T) hist[i] = 0u;
    __syncthreads();
    auto bin_of = [&](const klt_feat &ft) {
        if (ft.val < 0) return ORDER_BINS - 1;
        const int y = (int)ft.y;
        return y < 0 ? 0 : y > ORDER_BINS - 2 ? ORDER_BINS - 2 : y;
    };
    for (int i = tid; i < n; i += ORDER_T) atomicAdd(&hist[bin_of(in[i])], 1u);
    __syncthreads();
    // exclusive scan of the 4096 bins: 4 bins per thread, wave scan, then the 16 wave totals
    unsigned v[4], tsum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = hist[4 * tid + k]; tsum += v[k]; }
    unsigned inc = tsum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if ((tid & 63) >= d) inc += o;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int wv = 0; wv < (tid >> 6); wv++) base += wsum[wv];
    unsigned run = base + inc - tsum;
#pragma unroll
    for (int k = 0; k < 4; k++) { start[4 * tid + k] = run; run += v[k]; }
    __syncthreads();
    for (int i = tid; i < n; i += ORDER_T) order[atomicAdd(&start[bin_of(in[i])], 1u)] = (uint32_t)i;
}

// Iteration statistics from the per-feature aux words (only launched while statistics are being collected;
// per-feature atomics on a handful of shared counters would serialise the whole tracker).
__global__ __launch_bounds__(256) void track_stats_kernel(const klt_feat *__restrict__ in, const klt_feat *__restrict__ out,
                                                           int n, int nlevels, unsigned long long *stats)
{
    __shared__ unsigned int acc[1 + 2 * KLT_MAX_LEVELS];
    if (threadIdx.x < 1 + 2 * KLT_MAX_LEVELS) acc[threadIdx.x] = 0u;
    __syncthreads();
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < n && in[f].val >= 0) {
        atomicAdd(&acc[0], 1u);
        const uint32_t aux = (uint32_t)out[f].aux;
        for (int r = 0; r < nlevels; r++) {
            const uint32_t v = (aux >> (4 * r)) & 15u;
            if (v) {
                atomicAdd(&acc[1 + r], 1u);
                atomicAdd(&acc[1 + KLT_MAX_LEVELS + r], v - 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 1 + 2 * KLT_MAX_LEVELS && acc[threadIdx.x])
        atomicAdd(&stats[threadIdx.x], (unsigned long long)acc[threadIdx.x]);
}

// Constant-velocity prediction (klt_predict_cv_async): one record per lane, a 16-byte load of each list and a 16-byte store.
// guess = cur + (cur - prev), two f32 roundings per coordinate (no multiply: nothing to contract), for a feature that the last step tracked
// (cur.val == KLT_TRACKED) from a live one (prev.val >= 0); any other slot -- lost, or refilled by a replacement pass, whose val is its
// eigenvalue > 0 -- gets (-1, -1, -1, 0): no guess.
__global__ __launch_bounds__(256) void predict_cv_kernel(const klt_feat *__restrict__ prev, const klt_feat *__restrict__ cur,
                                                         klt_feat *__restrict__ guess, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 p = reinterpret_cast<const int4 *>(prev)[i], c = reinterpret_cast<const int4 *>(cur)[i];
    int4 o = make_int4(__float_as_int(-1.f), __float_as_int(-1.f), -1, 0);
    if (c.z == KLT_TRACKED && p.z >= 0) {
        const float cx = __int_as_float(c.x), cy = __int_as_float(c.y);
        o.x = __float_as_int(__fadd_rn(cx, __fsub_rn(cx, __int_as_float(p.x))));
        o.y = __float_as_int(__fadd_rn(cy, __fsub_rn(cy, __int_as_float(p.y))));
        o.z = 0;
    }
    reinterpret_cast<int4 *>(guess)[i] = o;
}

}  // namespace

void launch_predict_cv(hipStream_t s, const klt_feat *prev, const klt_feat *cur, klt_feat *guess, int n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(predict_cv_kernel, dim3((n + 255) / 256), dim3(256), 0, s, prev, cur, guess, n);
}

void launch_track_stats(hipStream_t s, const klt_feat *in, const klt_feat *out, int n, int nlevels, unsigned long long *stats)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(track_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n, nlevels, stats);
}

// Tracker kernels: track_kernel_quad (7x7 windows with long lists: four features per wavefront; 15x15 windows: one feature per
// wavefront; one 16-byte load per lane, image and footprint), track_kernel (one feature per wavefront, one sample per lane and round:
// every other window, short 7x7 lists).  All give bit-identical records.  Which of them a launch takes, with which grid and LDS:
// plan_track (track_plan.h).  The measured-slower generations in between (prefetching, per-sample loads with four features per
// wavefront, one pixel per lane) are recorded in profiles/README.md and live in the git history.
static_assert(LZ_FLOATS == TRACK_LAZY_FLOATS && LZE_FLOATS == TRACK_LAZY_ENTRY_FLOATS, "the plan's LDS sizes are these kernels'");

// The instantiation a plan names, of the plain (FB, GUESS false), forward-backward and motion-prior kernels
template <bool BATCH, bool FB, bool GUESS>
static void launch_track_t(hipStream_t s, const TrackPlan &p, const TrackGuessArgs &a)
{
    const TrackKernArgs<FB, GUESS> &ka = a;              // what the kernels take: the plain ones not the forward-backward fields, only those with a prior the guess list
    const dim3 grid(p.gx, p.gy), block(64);
    const unsigned lds = (unsigned)p.lds;
    constexpr int GW = GUESS ? GUESS_WAVES : 0;
    if (p.family == TRACK_FAMILY_QUAD7) {
        // (occupancy targets 5 / 6 for this kernel -- 96 / 80 VGPRs with 84 / 172 bytes of scratch per lane instead of 122 VGPRs -- were
        // measured again in round 3 on eight-pair launches, 10 000 wavefronts, where a fifth resident wavefront per SIMD could hide
        // latency: 112 / 199 us per launch against 87.5, cfg-4's 32-pair shard 0.535 / 0.687 ms against 0.495.  A scratch reload is a
        // vector memory operation and those return in order: it waits behind the footprint loads in flight, i.e. for the round trip
        // the extra wavefront was meant to hide.)
        // (the forward-backward instantiation is left without a cap as well -- an occupancy target of two is none for a kernel of 138
        // VGPRs, which three wavefronts per SIMD fit; its registers and scratch are in DESIGN.md section 9a)
        if constexpr (FB) klt_launch((track_kernel_quad<BATCH, 7, 2 + GW, false, true, GUESS>), grid, block, lds, s, ka);
        else if (p.tree) klt_launch((track_kernel_quad<BATCH, 7, 1 + GW, true, false, GUESS>), grid, block, lds, s, ka);
        else klt_launch((track_kernel_quad<BATCH, 7, 1 + GW, false, false, GUESS>), grid, block, lds, s, ka);
    } else if (p.family == TRACK_FAMILY_QUAD15) {
        // occupancy target 5 (96 VGPRs, 40 bytes of scratch per lane instead of 107 VGPRs): the 5000 wavefronts of cfg-3 are then
        // resident at once instead of in two rounds -- 57.9 -> 49.3 us.  (The 7x7 kernel loses from the same cap, see above.)
        // (forward-backward: occupancy target 4 -- 123 VGPRs, 36 bytes of scratch; at 5 the two passes' state costs 152 bytes of scratch per lane)
        if constexpr (FB) klt_launch((track_kernel_quad<BATCH, 15, 4 + GW, false, true, GUESS>), grid, block, lds, s, ka);
        else if (p.tree) klt_launch((track_kernel_quad<BATCH, 15, 5 + GW, true, false, GUESS>), grid, block, lds, s, ka);
        else klt_launch((track_kernel_quad<BATCH, 15, 5 + GW, false, false, GUESS>), grid, block, lds, s, ka);
    } else {
        for_window_class(p.maxk, p.wct, [&](auto maxk, auto wct) {
            klt_launch((track_kernel<maxk.value, wct.value, BATCH, FB, GUESS>), grid, block, lds, s, ka);
        });
    }
}

// ... and of the plain 7x7 quad kernels that read level 0 as compact images
template <bool BATCH>
static void launch_track_lazy_t(hipStream_t s, const TrackPlan &p, const TrackLazyArgs &a)
{
    const dim3 grid(p.gx, p.gy), block(64);
    if (p.entry) klt_launch((track_kernel_quad<BATCH, 7, 1 + LAZY_WAVES + ENTRY_WAVES>), grid, block, (unsigned)p.lds, s, a);
    else klt_launch((track_kernel_quad<BATCH, 7, 1 + LAZY_WAVES>), grid, block, (unsigned)p.lds, s, a);
}

// ------------------------------------------------------------------------------------------------------
// The reference's literal native boundary (setup.py:8-9), one call = one wavefront -- what the compat modules trackFeaturesUtils
// bind (pyfeaturetrack_amd/compat).  Separate (not interleaved) planes: the caller's own arrays.
namespace {

// extractImagePatchSlow, trackFeaturesUtils.pyx:14-51: w x w bilinear samples around (x, y); out[0] = 1 when the footprint leaves
// the image (the reference asserts, :35)
__global__ __launch_bounds__(64) void extract_patch_kernel(const float *__restrict__ img, int nc, int nr, float x, float y, int w,
                                                           float *__restrict__ patch, int *__restrict__ bad)
{
    const int hw = w / 2, n = w * w;
    const Bilinear b = make_bilinear(x, y);
    if (!(b.ix - hw >= 0 && b.iy - hw >= 0 && b.ix + hw + 2 <= nc && b.iy + hw + 2 <= nr)) {
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    if (threadIdx.x == 0) *bad = 0;
    for (int k = threadIdx.x; k < n; k += 64) {
        const size_t q = (size_t)(b.iy - hw + k / w) * nc + (b.ix - hw + k % w);
        patch[k] = sample(img + q, nc, b);
    }
}

// trackFeatureIterateCKLT, trackFeaturesUtils.pyx:393-459, on template patches the caller extracted: the Newton loop of track_level
// (same operations in the same order) without the template sampling, the post-loop tests and the status priority, which belong to
// _trackFeature (trackFeatures.py:67-136).  res = {x2, y2, status, iterations}
__global__ __launch_bounds__(64) void track_iterate_kernel(const float *__restrict__ t_gx, const float *__restrict__ t_gy,
                                                           const float *__restrict__ t_i, const float *__restrict__ i2,
                                                           const float *__restrict__ gx2, const float *__restrict__ gy2, int nc, int nr,
                                                           int w, float x2, float y2, float step, float small, float th,
                                                           int max_iterations, float *__restrict__ res)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, n = w * w, hw = w / 2, npad = track_npad(n);
    int iters = 0, status;
    const float one_plus_eps = 1.001f;
    for (;;) {
        if ((double)(x2 - (float)hw) < 0. || (float)nc - (x2 + (float)hw) < one_plus_eps ||
            (double)(y2 - (float)hw) < 0. || (float)nr - (y2 + (float)hw) < one_plus_eps) {       // :428-431
            status = KLT_OOB;
            break;
        }
        const Bilinear b2 = make_bilinear(x2, y2);
        const size_t base = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
        for (int k = lane; k < n; k += 64) {
            const size_t q = base + (size_t)(k / w) * nc + (k % w);
            const float diff = t_i[k] - sample(i2 + q, nc, b2);
            const float sx = t_gx[k] + sample(gx2 + q, nc, b2);
            const float sy = t_gy[k] + sample(gy2 + q, nc, b2);
            lds[k] = sx * sx;
            lds[npad + k] = sx * sy;
            lds[2 * npad + k] = sy * sy;
            lds[3 * npad + k] = diff * sx;
            lds[4 * npad + k] = diff * sy;
        }
        __syncthreads();
        float acc = 0.f;
        if (lane < 5) {
            const float *T = lds + lane * npad;
            for (int k = 0; k < n; k++) acc = acc + T[k];
        }
        __syncthreads();
        const float gxx = __shfl(acc, 0), gxy = __shfl(acc, 1), gyy = __shfl(acc, 2);
        const float ex = __shfl(acc, 3) * step, ey = __shfl(acc, 4) * step;
        float dx, dy;
        if (solve_step(gxx, gxy, gyy, ex, ey, small, dx, dy)) { status = KLT_SMALL_DET; break; }
        status = KLT_TRACKED;
        x2 = x2 + dx;
        y2 = y2 + dy;
        iters++;
        if (!((fabsf(dx) >= th || fabsf(dy) >= th) && iters < max_iterations)) break;
    }
    if (lane == 0) { res[0] = x2; res[1] = y2; res[2] = (float)status; res[3] = (float)iters; }
}

}  // namespace

void launch_extract_patch(hipStream_t s, const float *img, int nc, int nr, float x, float y, int w, float *patch, int *bad)
{
    hipLaunchKernelGGL(extract_patch_kernel, dim3(1), dim3(64), 0, s, img, nc, nr, x, y, w, patch, bad);
}

void launch_track_iterate(hipStream_t s, const float *t_gx, const float *t_gy, const float *t_i, const float *i2, const float *gx2,
                          const float *gy2, int nc, int nr, int w, float x2, float y2, float step, float small, float th,
                          int max_iterations, float *res)
{
    hipLaunchKernelGGL(track_iterate_kernel, dim3(1), dim3(64), (unsigned)track_lds_bytes(w * w), s, t_gx, t_gy, t_i, i2, gx2, gy2, nc, nr, w, x2, y2, step,
                       small, th, max_iterations, res);
}

// The tracker launch that plan_track (track_plan.h) chose for these arguments; it decides nothing.  kg, kd: the taps of the two gradient
// filters as TrackLazyArgs carries them (read by a lazy plan alone).  The feature order is (re)computed here whenever the arguments ask
// for it, whichever kernel consumes it.
void launch_track(hipStream_t s, const TrackPlan &p, const TrackGuessArgs &a, const double *kg, const double *kd)
{
    if (!p.launch || p.refusal) return;
    if (p.uses_order && a.order_refresh)
        hipLaunchKernelGGL(track_order_kernel, dim3(p.gy), dim3(ORDER_T), 0, s, a.in, p.batched ? a.pairs : nullptr, a.n, a.order);
    if (p.rule == TRACK_RULE_LIGHT) return launch_track_light_kernel(s, p, a);
    if (p.lazy) {
        TrackLazyArgs la;
        static_cast<TrackArgsBase &>(la) = a;
        for (int i = 0; i < 4; i++) { la.kg[i] = kg[i]; la.kd[i] = kd[i]; }
        return p.batched ? launch_track_lazy_t<true>(s, p, la) : launch_track_lazy_t<false>(s, p, la);
    }
    if (p.fb && p.guess) return launch_track_t<false, true, true>(s, p, a);      // (single-pair: no batched entry point takes a prior and the check together)
    if (p.fb) return p.batched ? launch_track_t<true, true, false>(s, p, a) : launch_track_t<false, true, false>(s, p, a);
    if (p.guess) return p.batched ? launch_track_t<true, false, true>(s, p, a) : launch_track_t<false, false, true>(s, p, a);
    return p.batched ? launch_track_t<true, false, false>(s, p, a) : launch_track_t<false, false, false>(s, p, a);
}
