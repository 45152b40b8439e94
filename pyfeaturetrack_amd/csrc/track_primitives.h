// The tracker's per-feature primitives, once: what track_kernels.hip, track_light_kernels.hip (the gain / bias tracker) and
// quality_kernels.hip all compute the same way.  Every function here encodes a rounding order of the reference -- FP64 bilinear weights
// with one f32 term, sequential f32 chains in row-major order, numpy's pairwise sum, un-fused products -- so there is one copy to fix.
// They were moved here from track_kernels.hip verbatim, and the device assembly of all three files was compared with that of the copies
// they replace (tools/kernel_regs.py's compile, -S): identical but for the per-compile id symbols and the mangled name of the one
// out-of-line function.  A change here is checked the same way.
#pragma once

#include <type_traits>

#include "klt_internal.h"

#pragma clang fp contract(off)

namespace {

struct Bilinear {
    double w00, w01, w10;
    float w11;
    int ix, iy;
};

// trackFeaturesUtils.pyx:23-31, :44-47
__device__ __forceinline__ Bilinear make_bilinear(float x, float y)
{
    Bilinear b;
    b.ix = (int)x;
    b.iy = (int)y;
    const float ax = (float)((double)x - (double)b.ix);
    const float ay = (float)((double)y - (double)b.iy);
    b.w00 = (1. - (double)ax) * (1. - (double)ay);
    b.w01 = (double)ax * (1. - (double)ay);
    b.w10 = (1. - (double)ax) * (double)ay;
    b.w11 = ax * ay;
    return b;
}

// ST = element stride of the plane: 1 for a plane of its own, KLT_PIX_STRIDE for one of the three planes of a level's pixel records (qg
// then points at the plane's own element of the pixel: image at +0, gradx at +1, grady at +2)
template <int ST = 1>
__device__ __forceinline__ float sample(const float *__restrict__ qg, int nc, const Bilinear &b)
{
    // the planes live in device memory: global loads (a flat load also counts as an LDS operation)
    const __attribute__((address_space(1))) float *q = (const __attribute__((address_space(1))) float *)qg;
    const float t4 = b.w11 * q[ST * (nc + 1)];
    double v = b.w00 * (double)q[0];
    v = v + b.w01 * (double)q[ST];
    v = v + b.w10 * (double)q[ST * nc];
    v = v + (double)t4;
    return (float)v;
}

// _solveEquation, trackFeaturesUtils.pyx:318-340: the step (dx, dy) from the five sums (ex, ey already times the step factor).
// Returns whether the determinant is too small, in which case the step means nothing (it is formed all the same: a division
// that nobody reads costs nothing, and the quad kernels divide before they look at the predicate).
__device__ __forceinline__ bool solve_step(float gxx, float gxy, float gyy, float ex, float ey, float small, float &dx, float &dy)
{
    const float p1 = gxx * gyy, p2 = gxy * gxy;
    const float det = p1 - p2;
    const float n1 = gyy * ex, n2 = gxy * ey, n3 = gxx * ey, n4 = gxy * ex;
    dx = (n1 - n2) / det;
    dy = (n3 - n4) / det;
    return det < small;
}

// (track_npad, the 16-byte aligned length of one of a window's five product arrays in LDS: track_plan.h)

// One product array added in the reference's row-major order (sequential f32 adds, trackFeaturesUtils.pyx:263-267, :296-302), read
// from LDS 16 bytes at a time: N terms, N known at compile time (a window size known at run time only: a plain loop over the terms).
//   PEEL == false: every quad carries the tests of its last three elements.  Unrolled completely they fold (7x7: 13 quads; the
//       peeled form measured 0.4 us slower there).
//   PEEL == true: whole quads without a test, the N % 4 tail on its own.  15x15 quad kernel: with the tests inside the partly
//       unrolled loop every quad paid three scalar compares and branches (13 M scalar next to 20 M vector instructions per launch):
//       49.0 -> 38.5 us.
template <int N, bool PEEL, int UNROLL>
__device__ __forceinline__ float chain_sum(const float4 *T4)
{
    float acc = 0.f;
    if (PEEL) {
#pragma unroll UNROLL
        for (int q = 0; q < N / 4; q++) {
            const float4 v = T4[q];
            acc = acc + v.x;
            acc = acc + v.y;
            acc = acc + v.z;
            acc = acc + v.w;
        }
        if (N % 4) {
            const float4 v = T4[N / 4];
            acc = acc + v.x;
            if (N % 4 > 1) acc = acc + v.y;
            if (N % 4 > 2) acc = acc + v.z;
        }
    } else {
#pragma unroll UNROLL
        for (int q = 0; q < (N + 3) / 4; q++) {
            const float4 v = T4[q];
            acc = acc + v.x;
            if (4 * q + 1 < N) acc = acc + v.y;
            if (4 * q + 2 < N) acc = acc + v.z;
            if (4 * q + 3 < N) acc = acc + v.w;
        }
    }
    return acc;
}

// numpy's pairwise summation of n floats in LDS (trackFeatures.py:124), computed by a group of lanes; the result is valid in
// its lane 0.  For a block of 8 <= n <= 128 numpy keeps eight running sums r[j] = a[j] + a[8 + j] + a[16 + j] + ... (each a
// sequential chain, independent of the others), folds them as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and then adds
// the n % 8 tail one by one.  Lanes 0..7 run the eight chains side by side and three shuffles do the fold: the same
// additions in the same order as the 1-lane loop, in 5 + 3 + tail steps instead of n.
// `s` = the lane's index within the summing group: the wavefront, or the lane group of a feature of the quad kernels (the result
// is then valid in the group's lane s == 0).
__device__ __forceinline__ float pairwise_block(const float *a, int n, int s)
{
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; i++) res = res + a[i];
        return res;
    }
    const int nn = n - (n % 8);
    float r = 0.f;
    if (s < 8) {
        r = a[s];
        for (int i = 8; i < nn; i += 8) r = r + a[i + s];
    }
    r = r + __shfl_down(r, 1);          // lanes 0, 2, 4, 6: r0 + r1, r2 + r3, r4 + r5, r6 + r7
    r = r + __shfl_down(r, 2);          // lanes 0, 4
    float res = r + __shfl_down(r, 4);  // lane 0
    for (int i = nn; i < n; i++) res = res + a[i];
    return res;
}

// ... of any n: numpy halves blocks of more than 128 elements (n2 = n / 2 rounded down to a multiple of 8)
template <int DEPTH>
__device__ __forceinline__ float pairwise_sum(const float *a, int n, int s)
{
    if (n <= 128) return pairwise_block(a, n, s);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum<DEPTH - 1>(a, n2, s) + pairwise_sum<DEPTH - 1>(a + n2, n - n2, s);
}
template <>
__device__ __forceinline__ float pairwise_sum<0>(const float *a, int n, int s)
{
    return pairwise_block(a, n < 128 ? n : 128, s);
}
// (track_level's call of it stays a function: inlined there, the run-time-n tree moved every track_kernel<*, 0, *, *> figure,
// <1, 0, false, false> from 61 to 80 VGPRs)
__device__ float pairwise_sum_wave(const float *a, int n, int lane) { return pairwise_sum<3>(a, n, lane); }

// A level of a pair's descriptor table.  The table is written by the host before the launch and never by a kernel, so it is read
// through the constant address space: scalar loads, the six plane pointers stay in SGPRs (as they do for a single-pair launch, whose
// levels travel in the kernarg segment).  Read as generic memory the pointers arrive in VGPRs (the compiler cannot rule out that the
// feature stores alias the table): 12 more vector registers, and flat loads through them.
__device__ __forceinline__ TrackLevel load_level(const TrackLevel *p)
{
    typedef const __attribute__((address_space(4))) TrackLevel *cptr;
    const cptr c = (cptr)p;
    TrackLevel lv;
    lv.i1 = c->i1; lv.gx1 = c->gx1; lv.gy1 = c->gy1;
    lv.i2 = c->i2; lv.gx2 = c->gx2; lv.gy2 = c->gy2;
    lv.nc = c->nc; lv.nr = c->nr;
    return lv;
}

__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The record a feature ends with, from the status of the last level it visited and its level-0 position (trackFeatures.py:288-308)
__device__ __forceinline__ klt_feat track_record(const TrackArgsBase &a, int val, float xout, float yout, uint32_t aux)
{
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
    return o;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The records of pixels q .. q + 3 of a level (klt_internal.h: image, gradx, grady per pixel): 48 contiguous bytes at byte offset 12 q,
// three 4-byte aligned 16-byte loads as raw buffer loads -- the record pointer is wavefront-uniform, so the descriptor sits in four
// SGPRs and the lane's 32-bit byte offset is the whole vector address (a plane is below 2 GB).  A global load of plane + q costs a
// 64-bit vector add per load and a register pair for the address; a flat load (what a pointer read from generic memory gives) also
// counts as an LDS operation.  Word 3 of the descriptor: data format 32 bits, nothing else (raw dwords).  The twelve values are
// unpacked in registers into the quads of the three planes.
__device__ __forceinline__ void load_records(const float *rec, unsigned q, f32x4 &im, f32x4 &gx, f32x4 &gy)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)rec, 0, 0x7fffffff, 0x00020000);
    const unsigned o = 12u * q;
    const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));          // i0 x0 y0 i1
    const f32x4 b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 16u, 0, 0));    // x1 y1 i2 x2
    const f32x4 c = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o + 32u, 0, 0));    // y2 i3 x3 y3
    im.x = a.x; im.y = a.w; im.z = b.z; im.w = c.y;
    gx.x = a.y; gx.y = b.x; gx.z = b.w; gx.w = c.z;
    gy.x = a.z; gy.y = b.y; gy.z = c.x; gy.w = c.w;
}

// the image values alone of pixels q .. q + 3 (the residue): four 4-byte loads
__device__ __forceinline__ f32x4 load_record_images(const float *rec, unsigned q)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)rec, 0, 0x7fffffff, 0x00020000);
    const unsigned o = 12u * q;
    f32x4 im;
    im.x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0));
    im.y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, o + 12u, 0, 0));
    im.z = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, o + 24u, 0, 0));
    im.w = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, o + 36u, 0, 0));
    return im;
}

// the four window samples of a lane from its quad `a`: pairs (a.x,a.y), (a.y,a.z), (a.z,a.w), (a.w, right neighbour) and the same
// pairs of the row below (QPR = quads per footprint row: the lane holding the quad below is QPR lanes up)
template <int QPR>
__device__ __forceinline__ void sample_quad(const f32x4 a, const Bilinear &b, float out[4])
{
    f32x4 lo;
    lo.x = __shfl_down(a.x, QPR); lo.y = __shfl_down(a.y, QPR); lo.z = __shfl_down(a.z, QPR); lo.w = __shfl_down(a.w, QPR);
    const float rx = __shfl_down(a.x, 1), dx = __shfl_down(a.x, QPR + 1);
    const float v00[4] = {a.x, a.y, a.z, a.w}, v01[4] = {a.y, a.z, a.w, rx};
    const float v10[4] = {lo.x, lo.y, lo.z, lo.w}, v11[4] = {lo.y, lo.z, lo.w, dx};
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const float t4 = b.w11 * v11[m];
        double d = b.w00 * (double)v00[m];
        d = d + b.w01 * (double)v01[m];
        d = d + b.w10 * (double)v10[m];
        d = d + (double)t4;
        out[m] = (float)d;
    }
}

// Level-0 gradients on demand (the LAZY kernels of track_kernels.hip), the arithmetic that does not depend on which lane does it: host
// and device text, so that tests/lazy_grad_dump.cpp holds it against the oracle's gradient planes without a GPU.  Both are corr_regs on
// seven widened values -- the FP64 expression and the operation order of the level-0 kernels without the centre-tap elision.
// One patch row's horizontal pass: NOUT + 6 consecutive samples of the smoothed image p[0 ..] give NOUT values of each filter, centred on
// p[3 ..]: derivative taps -> d, Gaussian taps -> e.  Every sample is widened once.
template <int NOUT>
__host__ __device__ __forceinline__ void lazy_row_h(const float *p, const TapRegs<7> &kg, const TapRegs<7> &kd, float *d, float *e)
{
    double w[NOUT + 6];
#pragma unroll
    for (int i = 0; i < NOUT + 6; i++) w[i] = (double)p[i];
#pragma unroll
    for (int j = 0; j < NOUT; j++) {
        d[j] = corr_regs<7, -1>(w + 3 + j, kd);
        e[j] = corr_regs<7, 1>(w + 3 + j, kg);
    }
}

// One footprint column's vertical pass down D (SYM = 1 with the Gaussian taps: gradx) or E (SYM = -1 with the derivative taps: grady):
// the column's NOUT + 6 consecutive values c[0 ..] give the NOUT pixels whose rows are centred on c[3 ..].  Every value is widened once.
template <int SYM, int NOUT>
__host__ __device__ __forceinline__ void lazy_col_v(const float *c, const TapRegs<7> &k, float *out)
{
    double w[NOUT + 6];
#pragma unroll
    for (int j = 0; j < NOUT + 6; j++) w[j] = (double)c[j];
#pragma unroll
    for (int j = 0; j < NOUT; j++) out[j] = corr_regs<7, SYM>(w + 3 + j, k);
}

// A window class of the one-feature-per-wavefront kernels (host; track_window_class of track_plan.h has the table) as integral
// constants: f(MAXK, WCT)
template <class F>
inline void for_window_class(int maxk, int wct, F &&f)
{
    using std::integral_constant;
    if (wct == 7) f(integral_constant<int, 1>{}, integral_constant<int, 7>{});
    else if (wct == 15) f(integral_constant<int, 4>{}, integral_constant<int, 15>{});
    else if (maxk == 1) f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
    else if (maxk == 2) f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
    else if (maxk == 4) f(integral_constant<int, 4>{}, integral_constant<int, 0>{});
    else if (maxk == 8) f(integral_constant<int, 8>{}, integral_constant<int, 0>{});
    else f(integral_constant<int, 16>{}, integral_constant<int, 0>{});
}

}  // namespace
