// consensus_primitives.h -- what the two consensus checks over feature lists share on the device (gfx950, wave64): the motion-model check
// (model_kernels.hip) and the epipolar check (epipolar_kernels.hip, section 9h).  Both read the candidates that
// model_gather_kernel wrote (32-byte records of centred (p, q)), pick samples with the same hash, and add their refit sums in the same
// 64 partials.  One copy of each primitive; everything is inlined into its callers.
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

}  // namespace consensus
