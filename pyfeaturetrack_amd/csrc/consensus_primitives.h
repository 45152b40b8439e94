// consensus_primitives.h -- what the consensus checks over feature lists share on the device (gfx950, wave64): the motion-model check
// (model_kernels.hip), the epipolar check (epipolar_kernels.hip, section 9h) and the homography check
// (homography_kernels.hip, section 9i).  All read the candidates that model_gather_kernel wrote (32-byte records of centred (p, q)), pick
// samples with the same hash, and add their refit sums in the same 64 partials; the last two also share the working coordinates and
// null9, the division-free null vector of an 8x9 matrix spread over a wavefront.  One copy of each primitive; everything is inlined
// into its callers.
#pragma once
#include "klt_internal.h"

namespace consensus {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

template <bool BATCH>
__device__ __forceinline__ ModelPair pair_of(const ModelArgs &a)
{
    if (!BATCH) return a.one;
    typedef const __attribute__((address_space(4))) ModelPair *cptr;
    const cptr c = (cptr)(a.pairs + blockIdx.y);
    ModelPair pr;
    pr.in = c->in; pr.out = c->out; pr.model = c->model; pr.cand = c->cand; pr.idx = c->idx; pr.scores = c->scores; pr.count = c->count;
    return pr;
}

__device__ __forceinline__ uint32_t mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// candidate number r_j of hypothesis h among m candidates, for a rule that draws PICKS candidates per hypothesis
template <uint32_t PICKS>
__device__ __forceinline__ int pick(uint32_t seed, uint32_t h, uint32_t j, int m)
{
    return (int)__umulhi(mix(seed ^ mix(PICKS * h + j)), (uint32_t)m);
}

struct Cand { double px, py, qx, qy; };

__device__ __forceinline__ Cand load_cand(const double *cand, int k)
{
    const f64x2 *c = reinterpret_cast<const f64x2 *>(cand) + 2 * (size_t)k;
    const f64x2 p = c[0], q = c[1];
    return Cand{p.x, p.y, q.x, q.y};
}

// U candidates k0 + stride * j + lane_or_thread, j = 0 .. U-1, all loads issued before the first is used; one beyond m is (0, 0, 0, 0), ok[j] false
template <int U>
__device__ __forceinline__ void load_ahead(const double *cand, int k0, int stride, int m, Cand (&c)[U], bool (&ok)[U])
{
#pragma unroll
    for (int j = 0; j < U; j++) {
        const int k = k0 + stride * j;
        ok[j] = k < m;
        c[j] = Cand{0., 0., 0., 0.};
        if (ok[j]) c[j] = load_cand(cand, k);
    }
}

// the 64 partials of a rule's sums, one per lane, folded into lane 0 (p[l] += p[l + w], l < w, w = 32 .. 1) and handed to every lane
__device__ __forceinline__ double fold64(double p)
{
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) p = p + __shfl_down(p, w);
    return __shfl(p, 0);
}

__device__ __forceinline__ int lane_rank(unsigned long long ballot)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// the best hypothesis of a workgroup of THREADS threads: the largest score, ties to the smallest h, as a key (score + 1) << 32 | ~h whose
// maximum does not depend on the reduction's order.  wave_key: THREADS / 64 entries of LDS; the caller synchronises once after the call
// (reduce_best_key) and then reads the result (best_key_of).
template <int THREADS>
__device__ __forceinline__ void reduce_best_key(const int *scores, int hypotheses, unsigned long long *wave_key)
{
    const int t = threadIdx.x;
    unsigned long long key = 0;
    for (int h = t; h < hypotheses; h += THREADS) {
        const unsigned long long k = (unsigned long long)(unsigned)(scores[h] + 1) << 32 | (0xffffffffu - (unsigned)h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned lo = __shfl_down((unsigned)key, o), hi = __shfl_down((unsigned)(key >> 32), o);
        const unsigned long long k = (unsigned long long)hi << 32 | lo;
        key = k > key ? k : key;
    }
    if ((t & 63) == 0) wave_key[t >> 6] = key;
}

template <int THREADS>
__device__ __forceinline__ unsigned long long best_key_of(const unsigned long long *wave_key)
{
    unsigned long long key = wave_key[0];
#pragma unroll
    for (int i = 1; i < THREADS / 64; i++) key = wave_key[i] > key ? wave_key[i] : key;
    return key;
}

// ---- what the epipolar check and the homography check share beyond that: working coordinates and the 8x9 null vector.  Every product
// and sum is its own statement, in the order of the rules in include/klt_gpu.h; nothing below may be contracted.
#pragma clang fp contract(off)

struct F9 { double f[9]; };                                          // (indexed by compile-time constants only)

__device__ __forceinline__ Cand working(Cand c, double s)
{
    c.px = c.px * s; c.py = c.py * s; c.qx = c.qx * s; c.qy = c.qy * s;
    return c;
}

template <int U>
__device__ __forceinline__ void load_working(const double *cand, int k0, int stride, int m, double s, Cand (&c)[U], bool (&ok)[U])
{
    load_ahead<U>(cand, k0, stride, m, c, ok);
#pragma unroll
    for (int j = 0; j < U; j++) c[j] = working(c[j], s);
}

// null9 (step 4 of the epipolar rule and of the homography rule, include/klt_gpu.h) on a matrix spread over the wavefront: `a` is
// A[lane >> 3][lane & 7], `a8` is A[lane >> 3][8].  All 64 lanes call
// it together; the result and f are the same in every lane.
__device__ __forceinline__ bool null9(double a, double a8, int lane, F9 &F)
{
    const int r = lane >> 3, c = lane & 7;
    int perm = lane;                                         // lanes 0 .. 8: the column of the input that stands at position `lane`
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const bool rows = r >= k;
        // the pivot: largest bits of |v|, then the smallest 9 row + column
        unsigned long long kb = 0;
        unsigned ki = 0;
        if (rows && c >= k) { kb = (unsigned long long)__double_as_longlong(fabs(a)); ki = 127u - (unsigned)(r * 9 + c); }
        if (rows) {
            const unsigned long long b8 = (unsigned long long)__double_as_longlong(fabs(a8));
            const unsigned i8 = 127u - (unsigned)(r * 9 + 8);
            if (b8 > kb || (b8 == kb && i8 > ki)) { kb = b8; ki = i8; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)kb, o), hi = __shfl_xor((unsigned)(kb >> 32), o), oi = __shfl_xor(ki, o);
            const unsigned long long ob = (unsigned long long)hi << 32 | lo;
            if (ob > kb || (ob == kb && oi > ki)) { kb = ob; ki = oi; }
        }
        const int ef = __builtin_amdgcn_readfirstlane((int)(kb >> 52));
        if (ef == 0 || ef == 0x7ff) return false;            // zero, subnormal or not finite (uniform: every lane holds the same key)
        const int at = __builtin_amdgcn_readfirstlane((int)(127u - ki));
        const int pr = at / 9, pc = at - 9 * pr;             // (a constant divisor: a multiplication)
        // rows k and pr, then columns k and pc, change places
        const int sr = r == k ? pr : (r == pr ? k : r);
        a = __shfl(a, sr * 8 + c);
        a8 = __shfl(a8, sr * 8 + c);
        if (pc < 8) {
            const int sc = c == k ? pc : (c == pc ? k : c);
            a = __shfl(a, r * 8 + sc);
        } else {
            const double was = __shfl(a, r * 8 + k);
            a = c == k ? a8 : a;
            a8 = was;
        }
        perm = __shfl(perm, lane == k ? pc : (lane == pc ? k : lane));
        // the remaining block times a power of two: the pivot P lands in 0.5 <= |P| < 1
        const double scale = __longlong_as_double((long long)(2045 - ef) << 52);
        if (rows && c >= k) a = a * scale;
        if (rows) a8 = a8 * scale;
        // A[i][j] = A[i][j] * P - A[k][j] * A[i][k]
        const double P = __shfl(a, 9 * k), rk = __shfl(a, k * 8 + c), rk8 = __shfl(a8, k * 8), ci = __shfl(a, r * 8 + k);
        if (r > k && c > k) {
            const double t1 = a * P, t2 = rk * ci;
            a = t1 - t2;
        }
        if (r > k) {
            const double t1 = a8 * P, t2 = rk8 * ci;
            a8 = t1 - t2;
        }
    }
    // back-substitution: lane j <= 8 holds x[j]
    double x = lane == 8 ? 1.0 : 0.0;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const double aj = __shfl(a, i * 8 + c), a88 = __shfl(a8, i * 8);
        const double aij = lane == 8 ? a88 : aj;             // lane j: A[i][j]
        const double term = aij * x;
        double sum = __shfl(term, i + 1);
#pragma unroll
        for (int j = i + 2; j <= 8; j++) {
            const double tj = __shfl(term, j);
            sum = sum + tj;
        }
        const double aii = __shfl(a, 9 * i);
        if (lane > i) x = x * aii;
        if (lane == i) x = -sum;
    }
    // f[perm[c]] = x[c]
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const unsigned long long who = __ballot(lane < 9 && perm == t);      // exactly one lane: perm is a permutation of 0 .. 8
        F.f[t] = __shfl(x, __ffsll((long long)who) - 1);
    }
    return true;
}

}  // namespace consensus
