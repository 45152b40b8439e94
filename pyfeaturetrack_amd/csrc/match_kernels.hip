// Brute-force Hamming matcher over binary descriptors (gfx950): klt_match_async.  The rule stands in include/klt_gpu.h ("descriptors",
// rule 2), the cut of the train set in describe_rule.h; DESIGN.md section 9n.  Integer arithmetic; no atomics: nothing depends on the
// order in which workgroups arrive.
//
//   match_kernel          a workgroup of one wavefront takes 64 records of `a`, one per lane with its eight words in registers, and
//                         streams its range (blockIdx.y) of `b` through LDS in tiles of 256 records.  Every lane reads the same LDS
//                         address at a time -- a broadcast, no bank conflict -- and keeps (best distance, best index, second distance).
//                         The same kernel runs with the roles exchanged for the cross-check.
//   match_resolve_kernel  one lane per query: merges the ranges (best = the minimum by (distance, index); second = the minimum of every
//                         range's second and of the losing ranges' best) and applies the outcome order of the rule.
#include "klt_internal.h"
#include "describe_rule.h"

namespace match_kernels {

using namespace kltapi;

constexpr int NONE = 257;                         // the distance of "no candidate"

__global__ __launch_bounds__(kMatchBlock) void match_kernel(MatchArgs a)
{
    __shared__ uint4 tile[kMatchTile * 3];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * kMatchBlock + lane;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0;
    if (i < a.na) {
        const uint4 *rec = reinterpret_cast<const uint4 *>(a.a + i);
        q0 = rec[0]; q1 = rec[1]; q2 = rec[2];
    }
    const bool described = i < a.na && (int)q2.x == 1;
    // the gate as bounds on the other record's centre (64-bit sums clamped to 32 bits: any int32 centre is compared exactly)
    int xlo = INT_MIN, xhi = INT_MAX, ylo = INT_MIN, yhi = INT_MAX;
    if (a.radius > 0) {
        const long long cx = (int)q2.z, cy = (int)q2.w, r = a.radius;
        xlo = (int)(cx - r < INT_MIN ? INT_MIN : cx - r); xhi = (int)(cx + r > INT_MAX ? INT_MAX : cx + r);
        ylo = (int)(cy - r < INT_MIN ? INT_MIN : cy - r); yhi = (int)(cy + r > INT_MAX ? INT_MAX : cy + r);
    }
    int lo, hi;
    match_range(a.nb, a.splits, (int)blockIdx.y, &lo, &hi);
    int best_d = NONE, best_j = -1, second = NONE;
    for (int base = lo; base < hi; base += kMatchTile) {
        const int cnt = hi - base < kMatchTile ? hi - base : kMatchTile;
        __syncthreads();                                     // (the previous tile has been read)
        const uint4 *src = reinterpret_cast<const uint4 *>(a.b + base);
        for (int r = lane; r < cnt * 3; r += kMatchBlock) tile[r] = src[r];
        __syncthreads();
        for (int r = 0; r < cnt; r++) {
            const uint4 t2 = tile[3 * r + 2];
            if ((int)t2.x != 1) continue;                    // (the same for every lane)
            const uint4 t0 = tile[3 * r], t1 = tile[3 * r + 1];
            const int d = __popc(q0.x ^ t0.x) + __popc(q0.y ^ t0.y) + __popc(q0.z ^ t0.z) + __popc(q0.w ^ t0.w) +
                          __popc(q1.x ^ t1.x) + __popc(q1.y ^ t1.y) + __popc(q1.z ^ t1.z) + __popc(q1.w ^ t1.w);
            const int tx = (int)t2.z, ty = (int)t2.w;
            const bool cand = described && tx >= xlo && tx <= xhi && ty >= ylo && ty <= yhi;
            if (cand) {
                if (d < best_d) { second = best_d; best_d = d; best_j = base + r; }      // (a tie stays with the lower index)
                else if (d < second) second = d;
            }
        }
    }
    if (i < a.na) a.part[(size_t)blockIdx.y * (size_t)a.na + i] = make_int4(best_d, best_j, second, 0);
}

// the ranges of one record merged, in the order of the ranges (rising indices): best by (distance, index), and the second distance
__device__ inline void merge_ranges(const int4 *part, int n, int splits, int i, int *best_d, int *best_j, int *second)
{
    int bd = NONE, bj = -1, sec = NONE;
    for (int k = 0; k < splits; k++) {
        const int4 p = part[(size_t)k * (size_t)n + i];
        if (p.y >= 0) {
            if (p.x < bd) { sec = sec < bd ? sec : bd; bd = p.x; bj = p.y; }
            else sec = sec < p.x ? sec : p.x;
        }
        sec = sec < p.z ? sec : p.z;
    }
    *best_d = bd; *best_j = bj; *second = sec;
}

__global__ __launch_bounds__(256) void match_resolve_kernel(MatchResolveArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nq) return;
    struct klt_match m;
    if (a.q[i].val != 1) {
        m.train = -1; m.distance = 0; m.second = 0; m.val = 0;
    } else {
        int d, j, s;
        merge_ranges(a.fwd, a.nq, a.splits, i, &d, &j, &s);
        m.train = j; m.distance = d; m.second = s;
        if (j < 0) {
            m.val = 2;                                       // (distance = second = 257)
        } else if (d > a.p.max_distance) {
            m.val = 3;
        } else if (a.p.ratio_num != 0 && !((long long)d * a.p.ratio_den < (long long)s * a.p.ratio_num)) {
            m.val = 4;
        } else {
            m.val = 1;
            if (a.p.cross_check) {
                int bd, bq, bs;
                merge_ranges(a.bwd, a.nt, a.rsplits, j, &bd, &bq, &bs);
                if (bq != i) m.val = 5;
            }
        }
    }
    *reinterpret_cast<int4 *>(a.out + i) = make_int4(m.train, m.distance, m.second, m.val);
}

}  // namespace match_kernels

void launch_match(hipStream_t s, const MatchArgs &a)
{
    using namespace match_kernels;
    const dim3 grid((unsigned)((a.na + kMatchBlock - 1) / kMatchBlock), (unsigned)a.splits), block(kMatchBlock);
    klt_launch(match_kernel, grid, block, 0, s, a);
}

void launch_match_resolve(hipStream_t s, const MatchResolveArgs &a)
{
    using namespace match_kernels;
    klt_launch(match_resolve_kernel, dim3((unsigned)((a.nq + 255) / 256)), dim3(256), 0, s, a);
}
