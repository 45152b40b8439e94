// crowd_kernels.hip -- the crowding check (not in the reference).  The rule stands in include/klt_gpu.h: among the
// tracked records of a list, ordered by age descending and list index ascending, a record is CROWDED iff an earlier KEPT one lies within
// r = min_distance - 1 pixels of it in x and in y.  Three launches, none reads a frame:
//   crowd_prepare_kernel  one lane per record: candidate or not, its pixel, its cell and its age in (CrowdCand, 16 bytes), the crowd record
//                         of a non-candidate; the same lanes clear the cell counts.
//   crowd_rank_kernel     one lane per record: a candidate takes its place in its cell (one returning atomic on the cell's count: the order
//                         inside a cell is arbitrary and nothing depends on it).
//   crowd_resolve_kernel  ONE workgroup of 1024 lanes per list, so that every wait is a workgroup barrier: turns the counts into offsets
//                         (a scan over the cells), groups the candidates by cell (no atomics: offset + place), then decides in rounds --
//                           kept, if every higher-priority neighbour is crowded; crowded, if any higher-priority neighbour is kept --
//                         until a workgroup-uniform test finds no candidate undecided, and writes the records.  The highest-priority
//                         undecided candidate is decided in every round, so the rounds are at most the candidates; a state never changes
//                         once set, so a lane may read a neighbour's state while its owner writes it (in-place rounds: what it sees is
//                         either undecided or final) and the outcome is the serial walk's, whatever the timing.
// Cells are squares of `side` > r pixels: every neighbour of a candidate lies in the 3 x 3 cells around its own, and the three cells of a
// cell row are one contiguous run of `sorted`.  The one workgroup is bound by latency, not by bytes, so what the neighbour loop reads for
// EVERY neighbour -- its pixel and its state -- lives in LDS for lists up to kCrowdLdsStates records (5 bytes each); age and record number
// are fetched for the few that cover.  Longer lists read pixels from `sorted` and keep states as ints in the context's scratch (read and
// written past the L1, which other lanes' stores do not update).
// Batched form: blockIdx.y selects the list from a table in device memory (CrowdPair), the mechanism of QualityPair.
#include "klt_internal.h"

namespace crowd_kernels {

constexpr int RECORD_THREADS = 256;
constexpr int RESOLVE_THREADS = 1024;
constexpr int RESOLVE_WAVES = RESOLVE_THREADS / 64;
enum : int { UNDECIDED = 0, KEPT = 1, CROWDED = 2 };

template <bool BATCH>
__device__ inline CrowdPair pair_of(const CrowdArgs &a)
{
    if (BATCH) return a.pairs[blockIdx.y];
    return a.one;
}

template <bool BATCH>
__global__ __launch_bounds__(RECORD_THREADS) void crowd_prepare_kernel(CrowdArgs a)
{
    const CrowdPair pr = pair_of<BATCH>(a);
    const int i = blockIdx.x * RECORD_THREADS + threadIdx.x;
    if (i < a.gx * a.gy) pr.cells[i] = 0;
    if (i >= a.n) return;
    const int4 raw = reinterpret_cast<const int4 *>(pr.out)[i];
    const float x = __int_as_float(raw.x), y = __int_as_float(raw.y);
    // f32 comparisons in front of any conversion: NaN and the infinities fail, -0.0 passes (ncols, nrows <= 65535 are exact in f32)
    const bool cand = raw.z == KLT_TRACKED && x >= 0.f && x < (float)a.ncols && y >= 0.f && y < (float)a.nrows;
    CrowdCand e;
    e.cell = -1; e.pos = 0; e.age = 0; e.idx = 0;
    if (cand) {
        const int px = (int)x, py = (int)y;
        int age = pr.prev ? pr.prev[i].age : 0;
        if (age < 0) age = 0;
        e.cell = (py / a.side) * a.gx + px / a.side;
        e.pos = (int)((unsigned)px | ((unsigned)py << 16));
        e.age = age;
    } else {
        reinterpret_cast<int4 *>(pr.crowd)[i] = make_int4(0, -1, 0, 0);
    }
    reinterpret_cast<int4 *>(pr.info)[i] = make_int4(e.cell, e.pos, e.age, e.idx);
}

// info[i].idx becomes the candidate's place in its cell
template <bool BATCH>
__global__ __launch_bounds__(RECORD_THREADS) void crowd_rank_kernel(CrowdArgs a)
{
    const CrowdPair pr = pair_of<BATCH>(a);
    const int i = blockIdx.x * RECORD_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const int cell = pr.info[i].cell;
    if (cell >= 0) pr.info[i].idx = atomicAdd(pr.cells + cell, 1);
}

// o before me in the rule's order: the older one, the lower index among equals (never true of a record and itself)
__device__ inline bool goes_first(int o_age, int o_idx, int me_age, int me_idx)
{
    return o_age > me_age || (o_age == me_age && o_idx < me_idx);
}

__device__ inline bool covers(int o_pos, int me_pos, int r)
{
    const int dx = (o_pos & 0xffff) - (me_pos & 0xffff), dy = (int)((unsigned)o_pos >> 16) - (int)((unsigned)me_pos >> 16);
    return dx <= r && -dx <= r && dy <= r && -dy <= r;
}

// what the neighbour loop reads of every neighbour: LDS for lists that fit, the scratch otherwise
template <bool LDS_STATE>
struct Neighbours {
    int *pos_lds;
    unsigned char *state_lds;
    const CrowdCand *sorted;
    int *state_mem;
    __device__ inline int pos(int k) const { return LDS_STATE ? pos_lds[k] : sorted[k].pos; }
    __device__ inline int get(int k) const
    {
        return LDS_STATE ? (int)state_lds[k] : __hip_atomic_load(state_mem + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ inline void set(int k, int v) const
    {
        if (LDS_STATE) state_lds[k] = (unsigned char)v;
        else __hip_atomic_store(state_mem + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ inline void init(int k, int p) const
    {
        if (LDS_STATE) pos_lds[k] = p;
        set(k, UNDECIDED);
    }
};

// the three runs of `sorted` that hold the 3 x 3 cells around `cell`, one per cell row (an empty run where the frame ends): all six
// offsets are fetched before any is used
__device__ inline void cell_runs(const CrowdArgs &a, const int *starts, int cell, int from[3], int to[3])
{
    const int cy = cell / a.gx, cx = cell - cy * a.gx;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < a.gx ? cx + 1 : a.gx - 1;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int yy = cy + d - 1, row = (yy < 0 ? 0 : yy >= a.gy ? a.gy - 1 : yy) * a.gx;
        from[d] = starts[row + x0];
        to[d] = starts[row + x1 + 1];
        if (yy < 0 || yy >= a.gy) to[d] = from[d];
    }
}

template <bool BATCH, bool LDS_STATE>
__global__ __launch_bounds__(RESOLVE_THREADS) void crowd_resolve_kernel(CrowdArgs a)
{
    __shared__ int pos_lds[LDS_STATE ? kCrowdLdsStates : 1];
    __shared__ unsigned char state_lds[LDS_STATE ? kCrowdLdsStates : 1];
    __shared__ int wave_total[RESOLVE_WAVES];
    __shared__ int pending_flag[3];
    const CrowdPair pr = pair_of<BATCH>(a);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, ncells = a.gx * a.gy;
    const Neighbours<LDS_STATE> nb{pos_lds, state_lds, pr.sorted, pr.state};
    if (tid < 3) pending_flag[tid] = 0;
    const long long t0 = wall_clock64();     // (100 MHz; lane 0's stamps behind the barriers give the phases' shares, a diagnostic)

    // counts -> where each cell's group begins: every lane a run of cells, the lanes' sums scanned over the workgroup
    const int per = (ncells + RESOLVE_THREADS - 1) / RESOLVE_THREADS;
    const int c0 = tid * per < ncells ? tid * per : ncells, c1 = c0 + per < ncells ? c0 + per : ncells;
    int mine = 0;
    for (int c = c0; c < c1; c++) mine += pr.cells[c];
    int incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int run = incl - mine, m = 0;
    for (int w = 0; w < RESOLVE_WAVES; w++) {
        const int t = wave_total[w];
        if (w < wave) run += t;
        m += t;
    }
    for (int c = c0; c < c1; c++) {
        pr.starts[c] = run;
        run += pr.cells[c];
    }
    if (tid == 0) pr.starts[ncells] = m;
    __threadfence();
    __syncthreads();

    // the candidates grouped by cell: where the cell's group begins + the candidate's place in it
#pragma unroll 4
    for (int i = tid; i < n; i += RESOLVE_THREADS) {
        const int4 e = reinterpret_cast<const int4 *>(pr.info)[i];
        if (e.x >= 0) {
            const int slot = pr.starts[e.x] + e.w;
            reinterpret_cast<int4 *>(pr.sorted)[slot] = make_int4(e.x, e.y, e.z, i);
            nb.init(slot, e.y);
        }
    }
    __threadfence();
    __syncthreads();

    const long long t1 = wall_clock64();
    int rounds = 0;
    for (;;) {
        int pending = 0;
        for (int k = tid; k < m; k += RESOLVE_THREADS) {
            if (nb.get(k) != UNDECIDED) continue;
            const int4 me = reinterpret_cast<const int4 *>(pr.sorted)[k];      // (cell, pos, age, record)
            int from[3], to[3];
            cell_runs(a, pr.starts, me.x, from, to);
            int verdict = KEPT;
            for (int d = 0; d < 3 && verdict != CROWDED; d++)
                for (int j = from[d]; j < to[d]; j++) {
                    if (!covers(nb.pos(j), me.y, a.r)) continue;
                    const CrowdCand o = pr.sorted[j];
                    if (!goes_first(o.age, o.idx, me.z, me.w)) continue;
                    const int s = nb.get(j);
                    if (s == KEPT) { verdict = CROWDED; break; }
                    if (s == UNDECIDED) verdict = UNDECIDED;
                }
            if (verdict != UNDECIDED) nb.set(k, verdict);
            else pending = 1;
        }
        // workgroup-uniform: is any candidate undecided?  Three flags in turn: the one of round r + 2 is cleared behind round r's barrier
        if (pending) pending_flag[rounds % 3] = 1;
        __threadfence();
        __syncthreads();
        const int any = pending_flag[rounds % 3];
        if (tid == 0) pending_flag[(rounds + 2) % 3] = 0;
        rounds++;
        if (!any) break;
        if (rounds > m) break;      // (cannot be: every round decides the first undecided candidate of the order.  Workgroup-uniform.)
    }

    const long long t2 = wall_clock64();
    for (int k = tid; k < m; k += RESOLVE_THREADS) {
        const int4 me = reinterpret_cast<const int4 *>(pr.sorted)[k];
        if (nb.get(k) == KEPT) {
            const int age = me.z < 0x7ffffffe ? me.z : 0x7ffffffe;
            reinterpret_cast<int4 *>(pr.crowd)[me.w] = make_int4(age + 1, -1, 1, 0);
            continue;
        }
        // the winner: the first kept candidate of the order that covers this one
        const int aux = pr.out[me.w].aux;
        int from[3], to[3];
        cell_runs(a, pr.starts, me.x, from, to);
        int best_age = 0, best_idx = -1;
        for (int d = 0; d < 3; d++)
            for (int j = from[d]; j < to[d]; j++) {
                if (!covers(nb.pos(j), me.y, a.r) || nb.get(j) != KEPT) continue;
                const CrowdCand o = pr.sorted[j];
                if (best_idx < 0 || goes_first(o.age, o.idx, best_age, best_idx)) { best_age = o.age; best_idx = o.idx; }
            }
        reinterpret_cast<int4 *>(pr.crowd)[me.w] = make_int4(0, best_idx, 2, 0);
        reinterpret_cast<int4 *>(pr.out)[me.w] = make_int4(__float_as_int(-1.f), __float_as_int(-1.f), KLT_CROWDED, aux);
    }
    __syncthreads();
    if (tid == 0) {
        pr.rounds[0] = rounds;
        const long long t3 = wall_clock64();
        pr.rounds[1] = (int)(t1 - t0); pr.rounds[2] = (int)(t2 - t1); pr.rounds[3] = (int)(t3 - t2);      // grouping, rounds, records
    }
}

template <bool BATCH>
static void launch_records(hipStream_t s, const CrowdArgs &a, int which)
{
    const unsigned lists = BATCH ? (unsigned)a.npairs : 1u;
    const int lanes = which == 0 && a.gx * a.gy > a.n ? a.gx * a.gy : a.n;
    const dim3 grid((lanes + RECORD_THREADS - 1) / RECORD_THREADS, lists);
    if (which == 0) klt_launch((crowd_prepare_kernel<BATCH>), grid, dim3(RECORD_THREADS), 0, s, a);
    else klt_launch((crowd_rank_kernel<BATCH>), grid, dim3(RECORD_THREADS), 0, s, a);
}

template <bool BATCH>
static void launch_resolve(hipStream_t s, const CrowdArgs &a)
{
    const unsigned lists = BATCH ? (unsigned)a.npairs : 1u;
    if (a.n <= kCrowdLdsStates) klt_launch((crowd_resolve_kernel<BATCH, true>), dim3(1, lists), dim3(RESOLVE_THREADS), 0, s, a);
    else klt_launch((crowd_resolve_kernel<BATCH, false>), dim3(1, lists), dim3(RESOLVE_THREADS), 0, s, a);
}

}  // namespace crowd_kernels

void launch_crowd_prepare(hipStream_t s, const CrowdArgs &a)
{
    if (a.pairs) crowd_kernels::launch_records<true>(s, a, 0); else crowd_kernels::launch_records<false>(s, a, 0);
}

void launch_crowd_rank(hipStream_t s, const CrowdArgs &a)
{
    if (a.pairs) crowd_kernels::launch_records<true>(s, a, 1); else crowd_kernels::launch_records<false>(s, a, 1);
}

void launch_crowd_resolve(hipStream_t s, const CrowdArgs &a)
{
    if (a.pairs) crowd_kernels::launch_resolve<true>(s, a); else crowd_kernels::launch_resolve<false>(s, a);
}
