// Gain / bias (lighting-insensitive) translational KLT tracker (gfx950): klt_set_light_params mode 1.  Not in the reference as code -- its
// trackFeaturesUtils.pyx:152-239 carries KLT 1.3.4's _computeIntensityDifferenceLightingInsensitive and
// _computeGradientSumLightingInsensitive as commented text, and trackFeatures.py:119-120 calls for them; tc.lighting_insensitive raises
// there and here.  The kernels below follow that text to the letter (DESIGN.md section 9d has the rule once more, with its reasons).
//
// THE RULE, per pyramid level and feature.  T_k, Tgx_k, Tgy_k: the template samples of image 1; S_k, Sgx_k, Sgy_k: the samples of image 2
// at the current (x2, y2); k row-major over the w x w window, n = w * w, nf = (float)n.  All arithmetic f32, one rounding per operation,
// nothing contracted; samples by the bilinear expression of the plain tracker (make_bilinear / sample).
//   sums       sum1 = SUM T_k, sq1 = SUM T_k*T_k, sum2 = SUM S_k, sq2 = SUM S_k*S_k: sequential f32 chains in row-major order, every product
//              one rounded multiply.  sum1 / sq1 once per level, sum2 / sq2 every iteration.
//   difference alpha = (float)sqrt((double)((sq1/nf) / (sq2/nf)));  beta = sum1/nf - alpha*(sum2/nf);  diff_k = (T_k - S_k*alpha) - beta
//   gradients  alpha_g = (float)sqrt((double)((sum1/nf) / (sum2/nf))) -- the ratio of the MEANS, which is what KLT 1.3.4 computes under the
//              names sum1_squared / sum2_squared (:223-227);  sx_k = Tgx_k + Sgx_k*alpha_g, sy_k likewise
//   step       the five product sums, _solveEquation, the step factor, both bounds tests, the iteration cap, the status priority,
//              retainTrackers and the record's border rule: the plain tracker's (track_level of track_kernels.hip, track_record)
//   residue    at the final position from |diff_k| with alpha and beta recomputed there, added with numpy's pairwise sum
//   degenerate sum1, sq1, sum2, sq2 are tested on their bits to be positive and finite (0 < bits <= 0x7f7fffff) before anything is computed
//              from them, then alpha and alpha_g to be finite; if not, the level ends with KLT_SMALL_DET and the position stays where it is
//              -- in the Newton loop and again before the residue.  The C text would go on with NaN positions.  For the same reason a step
//              (dx, dy) that is not finite (products that overflowed behind a huge but finite alpha) ends the level the same way: a NaN
//              passes every `<` of the bounds tests, and an address would be formed from it.
//
// (float)sqrt((double)q) of an f32 q is the correctly rounded f32 square root of q: rounding the 53-bit root once more to 24 bits cannot
// change the result for a square root (53 >= 2 * 24 + 2).  It is computed here WITHOUT the compiler's FP64 square-root expansion, which is
// built from fused multiply-adds: tests/test_host_and_abi.py allows the tracker's code objects the FMAs of IEEE f32 divisions and no
// others.  light_sqrt takes the hardware's approximate root and settles the last bits by exact FP64 comparisons.
//
// Bilinear, sample, chain_sum, pairwise_sum, solve_step, load_level, track_record, load_records and sample_quad are the plain tracker's,
// from track_primitives.h: the single copy, moved there verbatim with the device assembly of this file compared before and after.
// The namespace's name keeps "track_kernel" in the kernels' symbols, which is how the FMA test tells tracker code objects from others.
#include <cstdlib>

#include "klt_internal.h"
#include "track_primitives.h"

#pragma clang fp contract(off)

namespace track_kernel_light {

// ------------------------------------------------------------------------------------------------------ the gain / bias rule
// (float)sqrt((double)q) for an f32 q >= 0 (see the head of the file).  The hardware's FP64 root is good to about 24 bits: rounded to f32
// it is the correctly rounded root or a neighbour of it.  r is the correctly rounded root iff lo(r)^2 <= q <= hi(r)^2 with lo / hi the
// midpoints between r and its neighbours -- 25-bit numbers, whose squares (50 bits) and q are exact in FP64, so each comparison is exact;
// a root of an f32 is never such a midpoint (the square of a 25-bit odd mantissa does not fit 24 bits), so there are no ties.  Every round
// moves r one f32 towards the root; four rounds are more than the hardware's error needs.  q = 0, inf and NaN come back as they are
// (their neighbours' comparisons are all false).
__device__ __forceinline__ float light_sqrt(float q)
{
    const double d = (double)q;
    float r = (float)__builtin_amdgcn_sqrt(d);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t b = __float_as_uint(r);
        const float rp = __uint_as_float(b - 1u), rn = __uint_as_float(b + 1u);
        const double lo = ((double)rp + (double)r) * 0.5, hi = ((double)r + (double)rn) * 0.5;
        const float r0 = r;
        if (lo * lo > d) r = rp;
        if (hi * hi < d) r = rn;
        if (!(r0 > 0.f)) r = r0;             // 0 (and NaN): no neighbours to look at
    }
    return r;
}

__device__ __forceinline__ bool positive_finite(float v) { return __float_as_uint(v) - 1u < 0x7f7fffffu; }    // 0 < bits <= 0x7f7fffff
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct LightGain {
    float alpha, beta, alpha_g;
};

// alpha, beta and alpha_g from the four sums; false = a degenerate window (the level ends with KLT_SMALL_DET).  Sums that fail the test
// are replaced by 1 before anything is computed from them (the lane groups of the quad kernel go through this side by side, a feature
// whose window is degenerate among them: what is computed for it is never looked at).
__device__ __forceinline__ bool light_gain(float sum1, float sq1, float sum2, float sq2, float nf, LightGain &g)
{
    const bool pos = positive_finite(sum1) && positive_finite(sq1) && positive_finite(sum2) && positive_finite(sq2);
    if (!pos) { sum1 = 1.f; sq1 = 1.f; sum2 = 1.f; sq2 = 1.f; }
    const float q1 = sq1 / nf, q2 = sq2 / nf;
    g.alpha = light_sqrt(q1 / q2);
    const float m1 = sum1 / nf, m2 = sum2 / nf;
    const float am2 = g.alpha * m2;
    g.beta = m1 - am2;
    g.alpha_g = light_sqrt(m1 / m2);
    return pos && finite_bits(g.alpha) && finite_bits(g.alpha_g);
}

// diff_k = (T_k - S_k*alpha) - beta
__device__ __forceinline__ float light_diff(float t, float s, const LightGain &g)
{
    const float p = s * g.alpha;
    const float d = t - p;
    return d - g.beta;
}

// sx_k = Tgx_k + Sgx_k*alpha_g
__device__ __forceinline__ float light_gsum(float tg, float sg, const LightGain &g)
{
    const float p = sg * g.alpha_g;
    return tg + p;
}

// `narr` arrays of n terms in LDS, array j added by lane j in row-major order; the sum of array j is in lane j's result
template <int WCT>
__device__ __forceinline__ float chain_arrays(const float *lds, int npad, int n, int lane, int narr)
{
    float acc = 0.f;
    if (lane < narr) {
        const float *T = lds + lane * npad;
        if constexpr (WCT > 0) acc = chain_sum<WCT * WCT, false, (WCT <= 8 ? 16 : 4)>(reinterpret_cast<const float4 *>(T));
        else
            for (int k = 0; k < n; k++) acc = acc + T[k];
    }
    return acc;
}

// One level of one feature by its wavefront: track_level of track_kernels.hip with the rule above.  Lane l owns window samples l, l + 64,
// ...; an iteration has two chain phases on the same five LDS arrays -- sum2 / sq2 on lanes 0 and 1, then the five product sums on lanes
// 0..4.  WCT > 0: window size known at compile time; WCT == 0: any odd window up to 31.
template <int MAXK, int WCT>
__device__ int track_light_level(const TrackArgsBase &a, const TrackLevel &lv, float x1, float y1, float &x2r, float &y2r, float *lds,
                                 int lane, int &iters)
{
    const int w = WCT > 0 ? WCT : a.window, n = w * w, hw = w / 2;
    const int npad = track_npad(n);
    const int nc = lv.nc, nr = lv.nr;
    const float nf = (float)n;
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
            lds[k] = t_i[kk];
            lds[npad + k] = t_i[kk] * t_i[kk];
        }
    }
    // sum1, sq1: once per level
    __syncthreads();
    float acc = chain_arrays<WCT>(lds, npad, n, lane, 2);
    __syncthreads();
    const float sum1 = __shfl(acc, 0), sq1 = __shfl(acc, 1);

    float x2 = x2r, y2 = y2r;
    int status;
    const float one_plus_eps = 1.001f;
    LightGain g;
    for (;;) {
        // trackFeaturesUtils.pyx:428-431 (integer half-window, f32 arithmetic)
        if ((double)(x2 - (float)hw) < 0. || (float)nc - (x2 + (float)hw) < one_plus_eps ||
            (double)(y2 - (float)hw) < 0. || (float)nr - (y2 + (float)hw) < one_plus_eps) {
            status = KLT_OOB;
            break;
        }
        const Bilinear b2 = make_bilinear(x2, y2);
        const size_t base = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
        float s_i[MAXK], s_gx[MAXK], s_gy[MAXK];
        // first phase: the samples of image 2 and their squares
#pragma unroll
        for (int kk = 0; kk < MAXK; kk++) {
            const int k = lane + 64 * kk;
            s_i[kk] = s_gx[kk] = s_gy[kk] = 0.f;
            if (k < n) {
                const size_t q = base + off[kk];
                s_i[kk] = sample<KLT_PIX_STRIDE>(lv.i2 + KLT_PIX_STRIDE * q, nc, b2);
                s_gx[kk] = sample<KLT_PIX_STRIDE>(lv.gx2 + KLT_PIX_STRIDE * q, nc, b2);
                s_gy[kk] = sample<KLT_PIX_STRIDE>(lv.gy2 + KLT_PIX_STRIDE * q, nc, b2);
                lds[k] = s_i[kk];
                lds[npad + k] = s_i[kk] * s_i[kk];
            }
        }
        __syncthreads();
        acc = chain_arrays<WCT>(lds, npad, n, lane, 2);
        __syncthreads();
        const float sum2 = __shfl(acc, 0), sq2 = __shfl(acc, 1);
        if (!light_gain(sum1, sq1, sum2, sq2, nf, g)) { status = KLT_SMALL_DET; break; }      // degenerate window
        // second phase: the five product arrays
#pragma unroll
        for (int kk = 0; kk < MAXK; kk++) {
            const int k = lane + 64 * kk;
            if (k < n) {
                const float diff = light_diff(t_i[kk], s_i[kk], g);
                const float sx = light_gsum(t_gx[kk], s_gx[kk], g);
                const float sy = light_gsum(t_gy[kk], s_gy[kk], g);
                lds[k] = sx * sx;
                lds[npad + k] = sx * sy;
                lds[2 * npad + k] = sy * sy;
                lds[3 * npad + k] = diff * sx;
                lds[4 * npad + k] = diff * sy;
            }
        }
        __syncthreads();
        acc = chain_arrays<WCT>(lds, npad, n, lane, 5);
        __syncthreads();
        const float gxx = __shfl(acc, 0), gxy = __shfl(acc, 1), gyy = __shfl(acc, 2);
        const float ex = __shfl(acc, 3) * a.step, ey = __shfl(acc, 4) * a.step;
        float dx, dy;
        if (solve_step(gxx, gxy, gyy, ex, ey, a.small, dx, dy)) { status = KLT_SMALL_DET; break; }
        if (!(finite_bits(dx) && finite_bits(dy))) { status = KLT_SMALL_DET; break; }             // a step that is not finite
        status = KLT_TRACKED;
        x2 = x2 + dx;
        y2 = y2 + dy;
        iters++;
        if (!((fabsf(dx) >= a.th || fabsf(dy) >= a.th) && iters < a.max_iterations)) break;
    }
    x2r = x2;
    y2r = y2;

    // trackFeatures.py:110 -- Python floats: half-window 3.5, eps 1.001 as doubles
    const double x2d = (double)x2, y2d = (double)y2, hwd = a.half_window;
    if (x2d - hwd < 0.0 || (double)nc - (x2d + hwd) < 1.001 || y2d - hwd < 0.0 || (double)nr - (y2d + hwd) < 1.001)
        status = KLT_OOB;

    // residue, trackFeatures.py:118-125, from |diff_k| with alpha and beta of the final position
    if (status == KLT_TRACKED && a.use_max_residue) {
        const Bilinear b2 = make_bilinear(x2, y2);
        const size_t base = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
        float s_i[MAXK];
#pragma unroll
        for (int kk = 0; kk < MAXK; kk++) {
            const int k = lane + 64 * kk;
            s_i[kk] = 0.f;
            if (k < n) {
                s_i[kk] = sample<KLT_PIX_STRIDE>(lv.i2 + KLT_PIX_STRIDE * (base + off[kk]), nc, b2);
                lds[k] = s_i[kk];
                lds[npad + k] = s_i[kk] * s_i[kk];
            }
        }
        __syncthreads();
        acc = chain_arrays<WCT>(lds, npad, n, lane, 2);
        __syncthreads();
        const float sum2 = __shfl(acc, 0), sq2 = __shfl(acc, 1);
        if (!light_gain(sum1, sq1, sum2, sq2, nf, g)) status = KLT_SMALL_DET;
        else {
#pragma unroll
            for (int kk = 0; kk < MAXK; kk++) {
                const int k = lane + 64 * kk;
                if (k < n) lds[k] = fabsf(light_diff(t_i[kk], s_i[kk], g));
            }
            __syncthreads();
            float s = pairwise_sum_wave(lds, n, lane);
            __syncthreads();
            s = __shfl(s, 0);
            if (s / nf > a.max_residue) status = KLT_LARGE_RESIDUE;
        }
    }

    if (a.retain) return KLT_TRACKED;                                   // :127-129
    if (status == KLT_SMALL_DET || status == KLT_OOB || status == KLT_LARGE_RESIDUE) return status;
    if (iters >= a.max_iterations) return KLT_MAX_ITERATIONS;
    return KLT_TRACKED;
}

// One feature per wavefront, every pyramid level inside the launch; features in list order (no XCD-aware order: a.order is not looked at)
template <int MAXK, int WCT, bool BATCH>
__global__ __launch_bounds__(64) void track_light_kernel(TrackArgsBase a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= a.n) return;
    const TrackLevel *levels = BATCH ? a.pairs[blockIdx.y].lv : a.lv;
    const klt_feat *fin = BATCH ? a.pairs[blockIdx.y].in : a.in;
    klt_feat *fout = BATCH ? a.pairs[blockIdx.y].out : a.out;
    const klt_feat ft = fin[f];
    if (ft.val < 0) {                       // only live features are tracked, trackFeatures.py:253
        if (lane == 0) fout[f] = ft;
        return;
    }
    const int L = a.nlevels;
    // trackFeatures.py:255-265: position at the coarsest resolution (divisions by a power of two: exact)
    float xloc = ft.x, yloc = ft.y;
    for (int r = 0; r < L; r++) { xloc = xloc * a.inv_ss; yloc = yloc * a.inv_ss; }
    float xout = xloc, yout = yloc;
    int val = KLT_TRACKED;
    uint32_t aux = 0;       // 4 bits per level: 0 = level not visited, v = v-1 Newton iterations (saturating at 14)
    for (int r = L - 1; r >= 0; r--) {
        xloc = xloc * a.ss; yloc = yloc * a.ss; xout = xout * a.ss; yout = yout * a.ss;
        int it = 0;
        const TrackLevel lv = BATCH ? load_level(levels + r) : levels[r];
        val = track_light_level<MAXK, WCT>(a, lv, xloc, yloc, xout, yout, lds, lane, it);
        aux |= (uint32_t)(it < 14 ? it + 1 : 15) << (4 * r);
        if (val == KLT_SMALL_DET || val == KLT_OOB) break;             // :284-285
    }
    if (lane == 0) fout[f] = track_record(a, val, xout, yout, aux);
}

// ------------------------------------------------------------------------------------------------------
// 7x7 windows, four features per wavefront: track_kernel_quad<BATCH, 7, ...> of track_kernels.hip with the rule above -- the 8x8 footprint
// as 16 quads of four pixels, one 16-byte load per lane and image, per-feature predicates, a footprint whose integer corner has not moved
// is kept.  Every feature's arithmetic is track_light_level's, operation for operation.

template <bool BATCH>
__global__ __launch_bounds__(64) void track_light_quad(TrackArgsBase a)
{
    constexpr int W = 7, FPW = 4, LPF = 64 / FPW, QPR = (W + 1) / 4;
    constexpr int w = W, n = W * W, hw = W / 2, npad = track_npad(n);
    static_assert((W + 1) * QPR == LPF, "one quad per lane");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, g = lane / LPF, s = lane % LPF, glead = lane - s;
    const int f = FPW * blockIdx.x + g;
    const TrackLevel *levels = BATCH ? a.pairs[blockIdx.y].lv : a.lv;
    const klt_feat *fin = BATCH ? a.pairs[blockIdx.y].in : a.in;
    klt_feat *fout = BATCH ? a.pairs[blockIdx.y].out : a.out;
    const bool valid = f < a.n;
    const klt_feat ft = fin[valid ? f : a.n - 1];
    const bool tracked_feature = valid && ft.val >= 0;       // only live features are tracked, trackFeatures.py:253
    if (valid && ft.val < 0 && s == 0) fout[f] = ft;
    if (!__any(tracked_feature)) return;
    const int L = a.nlevels;
    float *const gl = lds + g * 5 * npad;                    // this feature's five arrays
    const int qr = s / QPR, qh = s % QPR;                    // my quad: footprint row qr, columns 4 qh .. 4 qh + 3
    const int k0 = qr * w + 4 * qh;                          // window index of my first sample (qr, 4 qh)
    const float one_plus_eps = 1.001f;
    const float nf = (float)n;
    bool inside[4];                                          // which of my four samples lie inside the window
#pragma unroll
    for (int m = 0; m < 4; m++) inside[m] = qr < w && 4 * qh + m < w;

    // `narr` arrays of this feature added by its lanes 0 .. narr - 1; lane j's result is the sum of array j
    auto chains = [&](int narr) {
        wave_lds_sync();
        float acc = 0.f;
        if (s < narr) acc = chain_sum<n, false, 16>(reinterpret_cast<const float4 *>(gl + s * npad));
        wave_lds_sync();
        return acc;
    };

    // trackFeatures.py:255-265
    float xloc = ft.x, yloc = ft.y;
    for (int r = 0; r < L; r++) { xloc = xloc * a.inv_ss; yloc = yloc * a.inv_ss; }
    float xout = xloc, yout = yloc;
    int val = KLT_TRACKED;
    uint32_t aux = 0;
    bool alive = tracked_feature;                            // still descending the pyramid

    for (int r = L - 1; r >= 0; r--) {
        if (!__any(alive)) break;
        const TrackLevel lv = BATCH ? load_level(levels + r) : levels[r];
        const int nc = lv.nc, nr = lv.nr;
        if (alive) { xloc = xloc * a.ss; yloc = yloc * a.ss; xout = xout * a.ss; yout = yout * a.ss; }

        // image-1 template (trackFeatures.py:102-104); a window that leaves image 1 ends the feature
        const Bilinear b1 = make_bilinear(xloc, yloc);
        const bool t_ok = b1.ix - hw >= 0 && b1.iy - hw >= 0 && b1.ix + hw + 2 <= nc && b1.iy + hw + 2 <= nr;
        const bool run = alive && t_ok;
        const unsigned q1 = run ? __umul24((unsigned)(b1.iy - hw + qr), (unsigned)nc) + (unsigned)(b1.ix - hw + 4 * qh) : 0u;
        f32x4 t_qi, t_qgx, t_qgy;
        load_records(lv.i1, q1, t_qi, t_qgx, t_qgy);

        // the first iteration's bounds test (trackFeaturesUtils.pyx:428-431) and footprint loads go out behind the template's
        int it = 0, status = KLT_OOB;
        float x2 = xout, y2 = yout;
        bool iterating = run;
        Bilinear b2;
        f32x4 s_qi = {0.f, 0.f, 0.f, 0.f}, s_qgx = s_qi, s_qgy = s_qi;
        unsigned q_held = ~0u;                               // element offset of the footprint quads in s_q*: none of this level yet
        auto request_footprint = [&]() {
            const bool oob = (double)(x2 - (float)hw) < 0. || (float)nc - (x2 + (float)hw) < one_plus_eps ||
                             (double)(y2 - (float)hw) < 0. || (float)nr - (y2 + (float)hw) < one_plus_eps;
            if (iterating && oob) { status = KLT_OOB; iterating = false; }
            b2 = make_bilinear(x2, y2);
            const unsigned q = __umul24((unsigned)(b2.iy - hw + qr), (unsigned)nc) + (unsigned)(b2.ix - hw + 4 * qh);
            if (iterating && q != q_held) {
                load_records(lv.i2, q, s_qi, s_qgx, s_qgy);
                q_held = q;
            }
        };
        request_footprint();

        float t_i[4], t_gx[4], t_gy[4];
        sample_quad<QPR>(t_qi, b1, t_i);
        sample_quad<QPR>(t_qgx, b1, t_gx);
        sample_quad<QPR>(t_qgy, b1, t_gy);

        // sum1, sq1: once per level
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (inside[m]) {
                gl[k0 + m] = t_i[m];
                gl[npad + k0 + m] = t_i[m] * t_i[m];
            }
        }
        float acc = chains(2);
        const float sum1 = __shfl(acc, glead), sq1 = __shfl(acc, glead + 1);

        LightGain gn;
        while (__any(iterating)) {
            const bool act = iterating;
            float s_i[4], s_gx[4], s_gy[4];
            sample_quad<QPR>(s_qi, b2, s_i);
            sample_quad<QPR>(s_qgx, b2, s_gx);
            sample_quad<QPR>(s_qgy, b2, s_gy);
            // first phase: sum2, sq2
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (inside[m]) {
                    gl[k0 + m] = s_i[m];
                    gl[npad + k0 + m] = s_i[m] * s_i[m];
                }
            }
            acc = chains(2);
            const float sum2 = __shfl(acc, glead), sq2 = __shfl(acc, glead + 1);
            const bool ok = light_gain(sum1, sq1, sum2, sq2, nf, gn);
            // second phase: the five product sums
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (inside[m]) {
                    const int k = k0 + m;
                    const float diff = light_diff(t_i[m], s_i[m], gn);
                    const float sx = light_gsum(t_gx[m], s_gx[m], gn);
                    const float sy = light_gsum(t_gy[m], s_gy[m], gn);
                    gl[k] = sx * sx;
                    gl[npad + k] = sx * sy;
                    gl[2 * npad + k] = sy * sy;
                    gl[3 * npad + k] = diff * sx;
                    gl[4 * npad + k] = diff * sy;
                }
            }
            acc = chains(5);
            const float gxx = __shfl(acc, glead), gxy = __shfl(acc, glead + 1), gyy = __shfl(acc, glead + 2);
            const float ex = __shfl(acc, glead + 3) * a.step, ey = __shfl(acc, glead + 4) * a.step;
            float dx, dy;
            const bool small_det = solve_step(gxx, gxy, gyy, ex, ey, a.small, dx, dy);
            const bool step_ok = ok && !small_det && finite_bits(dx) && finite_bits(dy);
            if (act && !step_ok) { status = KLT_SMALL_DET; iterating = false; }       // degenerate window, small determinant, step not finite
            if (act && step_ok) {
                status = KLT_TRACKED;
                x2 = x2 + dx;
                y2 = y2 + dy;
                it++;
                iterating = (fabsf(dx) >= a.th || fabsf(dy) >= a.th) && it < a.max_iterations;
            }
            if (__any(iterating)) request_footprint();
        }
        if (run) { xout = x2; yout = y2; }

        // trackFeatures.py:110 -- Python floats: half-window 3.5, eps 1.001 as doubles
        const double x2d = (double)x2, y2d = (double)y2, hwd = a.half_window;
        if (run && (x2d - hwd < 0.0 || (double)nc - (x2d + hwd) < 1.001 || y2d - hwd < 0.0 || (double)nr - (y2d + hwd) < 1.001))
            status = KLT_OOB;

        // residue, trackFeatures.py:118-125, from |diff_k| with alpha and beta of the final position
        const bool need_res = run && status == KLT_TRACKED && a.use_max_residue;
        if (__any(need_res)) {
            const Bilinear br = make_bilinear(x2, y2);
            const unsigned q = __umul24((unsigned)(br.iy - hw + qr), (unsigned)nc) + (unsigned)(br.ix - hw + 4 * qh);
            f32x4 r_qi = s_qi;                               // the last footprint, if the final position has the same integer corner
            if (need_res && q != q_held) r_qi = load_record_images(lv.i2, q);
            float s_i[4];
            sample_quad<QPR>(r_qi, br, s_i);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (inside[m]) {
                    gl[k0 + m] = s_i[m];
                    gl[npad + k0 + m] = s_i[m] * s_i[m];
                }
            }
            acc = chains(2);
            const float sum2 = __shfl(acc, glead), sq2 = __shfl(acc, glead + 1);
            const bool ok = light_gain(sum1, sq1, sum2, sq2, nf, gn);
#pragma unroll
            for (int m = 0; m < 4; m++)
                if (inside[m]) gl[k0 + m] = fabsf(light_diff(t_i[m], s_i[m], gn));
            wave_lds_sync();
            float sres = pairwise_sum<3>(gl, n, s);
            wave_lds_sync();
            sres = __shfl(sres, glead);
            if (need_res && !ok) status = KLT_SMALL_DET;
            else if (need_res && sres / nf > a.max_residue) status = KLT_LARGE_RESIDUE;
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
    if (tracked_feature && s == 0) fout[f] = track_record(a, val, xout, yout, aux);
}

template <bool BATCH>
static void launch_track_light_t(hipStream_t s, const TrackPlan &p, const TrackArgsBase &a)
{
    const dim3 grid(p.gx, p.gy), block(64);
    if (p.family == TRACK_FAMILY_QUAD7) return klt_launch((track_light_quad<BATCH>), grid, block, (unsigned)p.lds, s, a);
    for_window_class(p.maxk, p.wct, [&](auto maxk, auto wct) {
        klt_launch((track_light_kernel<maxk.value, wct.value, BATCH>), grid, block, (unsigned)p.lds, s, a);
    });
}

}  // namespace track_kernel_light

// The instantiation that a plan under klt_set_light_params mode 1 names (launch_track of track_kernels.hip calls this; the kernels stay in
// this file for their symbols' sake)
void launch_track_light_kernel(hipStream_t s, const TrackPlan &p, const TrackArgsBase &a)
{
    return p.batched ? track_kernel_light::launch_track_light_t<true>(s, p, a) : track_kernel_light::launch_track_light_t<false>(s, p, a);
}
