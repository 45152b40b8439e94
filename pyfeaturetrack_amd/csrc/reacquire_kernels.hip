// Track identities with re-acquisition of lost tracks (gfx950): klt_reacquire_begin_async / klt_reacquire_step_async.  The rule stands in
// include/klt_gpu.h ("track identities"); DESIGN.md section 9o.  Integer arithmetic only, no division by a run-time value (the ring is a
// mask), vector memory operations only, no atomics: nothing depends on the order in which wavefronts or workgroups arrive.
//
//   reacq_begin_kernel      the first ident row, the cleared bank, the counters.
//   reacq_classify_kernel   ONE workgroup: counts the deposits (L), expires the bank entries no deposit will overwrite, then walks the
//                           slots in chunks of 256 with stable ranks (__ballot + __popcll inside a wavefront, a prefix over the four
//                           wavefronts through LDS): writes the deposits of rank >= L - C into the ring and the fresh slots' descriptors
//                           and slot indices into a dense list; leaves the fresh count, L, h and the valid count in device memory.
//                           No bank entry is written by two threads: an entry a deposit overwrites is not expired first.
//   reacq_nearest_kernel    one wavefront per record of one side (bank entries: the rule's queries; fresh records: the cross-check), its
//                           eight words in registers, the lanes stride over the other side; (best d, best index, second) per lane in
//                           rising index order, then reduced over the wavefront by (d, index).  The grid is sized on the host (capacity,
//                           n); wavefronts at or beyond the device-side count leave.
//   reacq_assign_kernel     ONE workgroup: the slots that are not fresh, then the fresh list in chunks: a fresh record adopts the id of the
//                           bank entry that is its best, whose best it is, and that passes the distance and ratio tests (and clears that
//                           entry: one entry, one record, by the cross-check); the others are ranked in slot order for new ids.
#include "klt_internal.h"

namespace reacquire_kernels {

constexpr int NONE = 257;                         // the distance of "no candidate"

__device__ inline void store4(void *p, int x, int y, int z, int w) { *reinterpret_cast<int4 *>(p) = make_int4(x, y, z, w); }

// step 2 of the rule for slot s: continued / fresh / lost
__device__ inline void classes(const ReacquireArgs &a, int s, bool *cont, bool *fresh, bool *lost)
{
    const int had = reinterpret_cast<const int4 *>(a.prev)[s].w != 0;
    const int lv = a.list[s].val;
    *cont = had && lv == 0;
    *fresh = lv >= 0 && !*cont;
    *lost = had && !*cont;
}

__device__ inline bool deposits(const ReacquireArgs &a, int s)
{
    bool cont, fresh, lost;
    classes(a, s, &cont, &fresh, &lost);
    return lost && a.p[s].val == 1;
}

// the sum of v over the workgroup, in every thread (scratch: kReacqWaves words nobody else uses until the next barrier but one)
__device__ inline int block_sum(int v, int *scratch)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < kReacqWaves; w++) t += scratch[w];
    return t;
}

// stable ranks of the threads with `flag` in thread order: this thread's rank and the workgroup's count (scratch as above)
__device__ inline int block_rank(bool flag, int *scratch, int *count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    __syncthreads();
    if (lane == 0) scratch[wave] = __popcll(b);
    __syncthreads();
    int rank = __popcll(b & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < kReacqWaves; w++) {
        const int c = scratch[w];
        if (w < wave) rank += c;
        total += c;
    }
    *count = total;
    return rank;
}

__global__ __launch_bounds__(kReacqBlock) void reacq_begin_kernel(ReacquireArgs a)
{
    const int t = blockIdx.x * kReacqBlock + threadIdx.x;
    if (t < a.n) {
        if (a.list[t].val >= 0) store4(a.ident + t, t, 0, 0, 2);
        else store4(a.ident + t, -1, 0, 0, 0);
    }
    if (t < 4 * a.capacity) store4(reinterpret_cast<int4 *>(a.bank) + t, 0, 0, 0, 0);
    if (t < kReacqStateWords) a.state[t] = t == kReacqNextId ? a.n : 0;
}

__global__ __launch_bounds__(kReacqBlock) void reacq_classify_kernel(ReacquireArgs a)
{
    __shared__ int scratch[kReacqWaves];
    const int tid = threadIdx.x;
    const int C = a.capacity, mask = C - 1;
    const int h = a.state[kReacqHead];
    int mine = 0;
    for (int s = tid; s < a.n; s += kReacqBlock) mine += deposits(a, s) ? 1 : 0;
    const int L = block_sum(mine, scratch);
    const int first = L > C ? L - C : 0;
    // the bank: an entry at ring offset < L is overwritten below (every entry when L >= C); the others expire or stay
    int4 *bank4 = reinterpret_cast<int4 *>(a.bank);
    int valid = 0;
    for (int e = tid; e < C; e += kReacqBlock) {
        if (((e - h) & mask) < L) { valid++; continue; }
        const int4 tail = bank4[4 * e + 3];                  // id, last_seen, valid, pad
        if (tail.z != 1) continue;
        if (a.k - tail.y - 1 > a.max_gap) {
            for (int w = 0; w < 4; w++) store4(bank4 + 4 * e + w, 0, 0, 0, 0);
        } else {
            valid++;
        }
    }
    valid = block_sum(valid, scratch);
    int dep_base = 0, fresh_base = 0;
    for (int base = 0; base < a.n; base += kReacqBlock) {    // (uniform bounds: every thread reaches every barrier)
        const int s = base + tid;
        bool cont = false, fresh = false, lost = false;
        if (s < a.n) classes(a, s, &cont, &fresh, &lost);
        const bool dep = lost && a.p[s].val == 1;
        int nd, nf;
        const int rd = dep_base + block_rank(dep, scratch, &nd);
        const int rf = fresh_base + block_rank(fresh, scratch, &nf);
        if (dep && rd >= first) {
            const int4 *src = reinterpret_cast<const int4 *>(a.p + s);
            int4 *dst = bank4 + 4 * ((h + rd) & mask);
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            store4(dst + 3, reinterpret_cast<const int4 *>(a.prev)[s].x, a.k - 1, 1, 0);
        }
        if (fresh) {
            const int4 *src = reinterpret_cast<const int4 *>(a.q + s);
            int4 *dst = reinterpret_cast<int4 *>(a.fresh_desc + rf);
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            a.fresh_slot[rf] = s;
        }
        dep_base += nd; fresh_base += nf;
    }
    __syncthreads();                                         // (every thread has read the head)
    if (tid == 0) {
        a.state[kReacqHead] = (h + L) & mask;
        a.state[kReacqValid] = valid;
        a.state[kReacqFresh] = fresh_base;
        a.state[kReacqLost] = L;
    }
}

template <bool OF_BANK>
__global__ __launch_bounds__(kReacqBlock) void reacq_nearest_kernel(ReacquireArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kReacqWaves + (threadIdx.x >> 6);
    const int nfresh = a.state[kReacqFresh];
    const int na = OF_BANK ? a.capacity : nfresh, nb = OF_BANK ? nfresh : a.capacity;
    if (i >= na) return;                                     // (the same for the whole wavefront; the kernel has no barrier)
    const uint4 *bank = reinterpret_cast<const uint4 *>(a.bank), *fresh = reinterpret_cast<const uint4 *>(a.fresh_desc);
    const uint4 *rec = OF_BANK ? bank + 4 * i : fresh + 3 * i;
    const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
    bool described = (int)q2.x == 1;
    if (OF_BANK) described = described && (int)rec[3].z == 1;
    // the gate as bounds on the other record's centre (64-bit sums clamped to 32 bits: any int32 centre is compared exactly)
    int xlo = INT_MIN, xhi = INT_MAX, ylo = INT_MIN, yhi = INT_MAX;
    if (a.mp.radius > 0) {
        const long long cx = (int)q2.z, cy = (int)q2.w, r = a.mp.radius;
        xlo = (int)(cx - r < INT_MIN ? INT_MIN : cx - r); xhi = (int)(cx + r > INT_MAX ? INT_MAX : cx + r);
        ylo = (int)(cy - r < INT_MIN ? INT_MIN : cy - r); yhi = (int)(cy + r > INT_MAX ? INT_MAX : cy + r);
    }
    int best_d = NONE, best_j = INT_MAX, second = NONE;
    if (described) {
        for (int j = lane; j < nb; j += 64) {
            const uint4 *t = OF_BANK ? fresh + 3 * j : bank + 4 * j;
            const uint4 t2 = t[2];
            bool cand = (int)t2.x == 1 && (int)t2.z >= xlo && (int)t2.z <= xhi && (int)t2.w >= ylo && (int)t2.w <= yhi;
            if (!OF_BANK) cand = cand && (int)t[3].z == 1;
            if (!cand) continue;
            const uint4 t0 = t[0], t1 = t[1];
            const int d = __popc(q0.x ^ t0.x) + __popc(q0.y ^ t0.y) + __popc(q0.z ^ t0.z) + __popc(q0.w ^ t0.w) +
                          __popc(q1.x ^ t1.x) + __popc(q1.y ^ t1.y) + __popc(q1.z ^ t1.z) + __popc(q1.w ^ t1.w);
            if (d < best_d) { second = best_d; best_d = d; best_j = j; }         // (a tie stays with the lower index)
            else if (d < second) second = d;
        }
    }
    // over the wavefront by (d, index); the loser's best is a candidate for the second distance.  No two lanes hold the same index
    // except INT_MAX with d = 257 ("none"), which neither side takes
    for (int o = 32; o; o >>= 1) {
        const int od = __shfl_xor(best_d, o), oj = __shfl_xor(best_j, o), os = __shfl_xor(second, o);
        const bool take = od < best_d || (od == best_d && oj < best_j);
        const int loser = take ? best_d : od;
        second = second < os ? second : os;
        second = second < loser ? second : loser;
        if (take) { best_d = od; best_j = oj; }
    }
    if (lane == 0) store4((OF_BANK ? a.bank_best : a.fresh_best) + i, best_d, best_j == INT_MAX ? -1 : best_j, second, 0);
}

__global__ __launch_bounds__(kReacqBlock) void reacq_assign_kernel(ReacquireArgs a)
{
    __shared__ int scratch[kReacqWaves];
    const int tid = threadIdx.x;
    const int nfresh = a.state[kReacqFresh], next_id = a.state[kReacqNextId], valid = a.state[kReacqValid];
    for (int s = tid; s < a.n; s += kReacqBlock) {
        bool cont, fresh, lost;
        classes(a, s, &cont, &fresh, &lost);
        if (cont) store4(a.ident + s, reinterpret_cast<const int4 *>(a.prev)[s].x, 0, 0, 1);
        else if (!fresh) store4(a.ident + s, -1, 0, 0, 0);
    }
    int4 *bank4 = reinterpret_cast<int4 *>(a.bank);
    int new_base = 0;
    for (int base = 0; base < nfresh; base += kReacqBlock) { // (uniform bounds)
        const int f = base + tid;
        bool is_new = false;
        int s = 0;
        if (f < nfresh) {
            s = a.fresh_slot[f];
            const int i = a.fresh_best[f].y;                 // the record's best bank entry (the cross-check's side)
            is_new = true;
            if (i >= 0) {
                const int4 b = a.bank_best[i];               // the entry's best record, its distance, the second distance
                if (b.y == f && b.x <= a.mp.max_distance &&
                    (a.mp.ratio_num == 0 || (long long)b.x * a.mp.ratio_den < (long long)b.z * a.mp.ratio_num)) {
                    const int4 tail = bank4[4 * i + 3];
                    store4(a.ident + s, tail.x, a.k - tail.y - 1, b.x, 3);
                    for (int w = 0; w < 4; w++) store4(bank4 + 4 * i + w, 0, 0, 0, 0);
                    is_new = false;
                }
            }
        }
        int cnt;
        const int r = new_base + block_rank(is_new, scratch, &cnt);
        if (is_new) store4(a.ident + s, next_id + r, 0, 0, 2);
        new_base += cnt;
    }
    __syncthreads();                                         // (every thread has read the counters)
    if (tid == 0) {
        a.state[kReacqNextId] = next_id + new_base;
        a.state[kReacqValid] = valid - (nfresh - new_base);
    }
}

}  // namespace reacquire_kernels

void launch_reacquire_begin(hipStream_t s, const ReacquireArgs &a)
{
    using namespace reacquire_kernels;
    const int work = a.n > 4 * a.capacity ? a.n : 4 * a.capacity;
    klt_launch(reacq_begin_kernel, dim3((unsigned)((work + kReacqBlock - 1) / kReacqBlock)), dim3(kReacqBlock), 0, s, a);
}

void launch_reacquire_classify(hipStream_t s, const ReacquireArgs &a)
{
    using namespace reacquire_kernels;
    klt_launch(reacq_classify_kernel, dim3(1), dim3(kReacqBlock), 0, s, a);
}

void launch_reacquire_nearest(hipStream_t s, const ReacquireArgs &a, bool of_bank)
{
    using namespace reacquire_kernels;
    const int records = of_bank ? a.capacity : a.n;
    const dim3 grid((unsigned)((records + kReacqWaves - 1) / kReacqWaves)), block(kReacqBlock);
    if (of_bank) klt_launch(reacq_nearest_kernel<true>, grid, block, 0, s, a);
    else klt_launch(reacq_nearest_kernel<false>, grid, block, 0, s, a);
}

void launch_reacquire_assign(hipStream_t s, const ReacquireArgs &a)
{
    using namespace reacquire_kernels;
    klt_launch(reacq_assign_kernel, dim3(1), dim3(kReacqBlock), 0, s, a);
}
