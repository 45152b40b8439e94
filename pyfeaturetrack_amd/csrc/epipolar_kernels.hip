// Epipolar check (gfx950, wave64): klt_epipolar_check_async.  Three launches in stream order read two feature lists, find the frame pair's
// fundamental matrix by a seeded consensus search over eight-point hypotheses with one least-squares refit, and turn every tracked feature
// off its epipolar line into (-1, -1, KLT_EPIPOLAR_OUTLIER, aux).  Nothing here reads a frame.  THE RULE stands in include/klt_gpu.h
// ("epipolar check"), word for word what this file computes; DESIGN.md section 9h has it with its reasons, tests/epipolar_expected.py is
// its numpy restatement and the device equals that bit for bit.
//
// Everything is FP64 with one rounding per operation in the header's order, `+`, `-` and `*` only, no `/` or `%` by a run-time integer;
// every product and sum below is its own statement or parenthesis, and contraction is off.
//
//   (candidates)             model_gather_kernel of the motion-model check, unchanged, on this check's own scratch: centred (p, q); the
//                            kernels here multiply by s = 2^-k on load (exact).
//   epipolar_score_kernel    one wavefront per hypothesis, four per workgroup.  The 8x9 matrix of the eight picks lives in registers, one
//                            entry per lane (lane l: row l >> 3, column l & 7; the ninth column rides along in a second register, the
//                            same value in the eight lanes of a row).  null9 moves entries between lanes by __shfl alone: the pivot's
//                            run-time position never indexes an array, so nothing goes to scratch.  The pivot search is a butterfly
//                            maximum of the key (bits of |v|, 127 - (9 row + column)): its order does not matter.  Then lanes stride over
//                            the candidates as in model_score_kernel; one int32 score per hypothesis.
//   epipolar_decide_kernel   one workgroup per pair.  Argmax as in model_decide_kernel.  Wavefront 0 redoes the best hypothesis and hands
//                            it round through LDS; the eight wavefronts share the 45 sums, every one over all candidates -- lane l IS
//                            partial l of the rule, folded by __shfl_down --; wavefront 0 takes out row g, runs null9 once more and
//                            publishes the final model through LDS; then all eight wavefronts test every candidate, scatter the
//                            outlier records (one 16-byte store each) and count; thread 0 writes the 96-byte model record.
// Batched form: blockIdx.y selects the pair from a table of ModelPair in device memory.
#include "consensus_primitives.h"

#pragma clang fp contract(off)

namespace epipolar_kernels {

using namespace consensus;

constexpr int SCORE_WAVES = 4;
constexpr int DECIDE_THREADS = 512;
constexpr int SCORE_AHEAD = 4, SUM_AHEAD = 8, FINAL_AHEAD = 4;      // candidates a lane loads before it uses the first

// step 5 of the rule: the Sampson distance, cross-multiplied
__device__ __forceinline__ bool is_inlier(const F9 &F, double t2, const Cand &c)
{
    const double *f = F.f;
    const double u0 = f[0] * c.px, u1 = f[1] * c.py, u2 = f[3] * c.px, u3 = f[4] * c.py, u4 = f[6] * c.px, u5 = f[7] * c.py;
    const double a0 = (u0 + u1) + f[2], a1 = (u2 + u3) + f[5], a2 = (u4 + u5) + f[8];
    const double v0 = f[0] * c.qx, v1 = f[3] * c.qy, v2 = f[1] * c.qx, v3 = f[4] * c.qy;
    const double b0 = (v0 + v1) + f[6], b1 = (v2 + v3) + f[7];
    const double r0 = a0 * c.qx, r1 = a1 * c.qy;
    const double r = (r0 + r1) + a2;
    const double d0 = a0 * a0, d1 = a1 * a1, d2 = b0 * b0, d3 = b1 * b1;
    const double den = ((d0 + d1) + d2) + d3;
    const double rr = r * r, lim = t2 * den;
    return rr <= lim;                                        // (NaN fails)
}

// entry (row lane >> 3, column lane & 7) of the row of correspondence c (step 3); the ninth column is 1.0.  Every entry is one product
// of q.x, q.y or 1.0 with p.x, p.y or 1.0, and a product with 1.0 is exact.
__device__ __forceinline__ double row_entry(const Cand &c, int col)
{
    const double l = col < 3 ? c.qx : (col < 6 ? c.qy : 1.0);
    const bool x = col == 0 || col == 3 || col == 6, y = col == 1 || col == 4 || col == 7;
    const double r = x ? c.px : (y ? c.py : 1.0);
    return l * r;
}

// steps 2 to 4 for hypothesis h: the eight rows of its picks, one entry per lane, and their null vector
__device__ __forceinline__ bool hypothesis(const ModelPair &pr, uint32_t seed, int h, int m, double s, int lane, F9 &F)
{
    const Cand c = working(load_cand(pr.cand, pick<8>(seed, (uint32_t)h, (uint32_t)(lane >> 3), m)), s);
    return null9(row_entry(c, lane & 7), 1.0, lane, F);
}

template <bool BATCH>
__global__ __launch_bounds__(64 * SCORE_WAVES) void epipolar_score_kernel(EpipolarArgs e)
{
    const ModelArgs &a = e.m;
    const ModelPair pr = pair_of<BATCH>(a);
    const int lane = threadIdx.x & 63;
    const int h = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6)));
    if (h >= a.hypotheses) return;
    const int m = *pr.count;
    if (m < a.min_inliers) return;                           // no model: the decision does not look at the scores
    F9 F;
    int score = -1;
    if (hypothesis(pr, a.seed, h, m, e.s, lane, F)) {
        score = 0;
        for (int k0 = 0; k0 < m; k0 += 64 * SCORE_AHEAD) {  // (a count: the order of the candidates does not matter)
            Cand c[SCORE_AHEAD];
            bool ok[SCORE_AHEAD];
            load_working<SCORE_AHEAD>(pr.cand, k0 + lane, 64, m, e.s, c, ok);
#pragma unroll
            for (int j = 0; j < SCORE_AHEAD; j++) score += __popcll(__ballot(ok[j] && is_inlier(F, a.t2, c[j])));
        }
    }
    if (lane == 0) pr.scores[h] = score;
}

__device__ __forceinline__ void write_model(klt_epipolar_model *dst, const F9 &F, int valid, int m, int n_inliers, int hyp, int hyp_inliers,
                                            int size)
{
    klt_epipolar_model r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.f[i] = F.f[i];
    r.valid = valid; r.n_candidates = m; r.n_inliers = n_inliers; r.hypothesis = hyp; r.hypothesis_inliers = hyp_inliers; r.pad = size;
    *dst = r;
}

// The sums number W, W + 8, W + 16, ... of the 45 (counted along the upper triangle of M, row by row) over the inliers of H, added by ONE
// wavefront over all candidates -- lane l is partial l of the rule, candidates l, l + 64, ... in increasing k --, folded, into sums[].
// Eight wavefronts share the 45 sums: each sum is added exactly as the rule says, and no wavefront holds more than six accumulators.
template <int W>
__device__ __forceinline__ void add_sums(const ModelPair &pr, const F9 &H, double t2, double s, int m, int lane, double *sums)
{
    constexpr int N = (45 - W + 7) / 8;
    double S[N];
#pragma unroll
    for (int q = 0; q < N; q++) S[q] = 0.;
    for (int k0 = 0; k0 < m; k0 += 64 * SUM_AHEAD) {
        Cand cs[SUM_AHEAD];
        bool ok[SUM_AHEAD];
        load_working<SUM_AHEAD>(pr.cand, k0 + lane, 64, m, s, cs, ok);
#pragma unroll
        for (int j = 0; j < SUM_AHEAD; j++) {
            const Cand c = cs[j];
            if (ok[j] && is_inlier(H, t2, c)) {
                double v[9];
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = row_entry(c, i);
                v[8] = 1.0;
                int u = 0;
#pragma unroll
                for (int i = 0; i < 9; i++)
#pragma unroll
                    for (int jj = i; jj < 9; jj++, u++)
                        if (u % 8 == W) {
                            const double term = v[i] * v[jj];
                            S[u / 8] = S[u / 8] + term;
                        }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < N; q++) {
        const double f = fold64(S[q]);
        if (lane == 0) sums[W + 8 * q] = f;
    }
}

template <bool BATCH>
__global__ __launch_bounds__(DECIDE_THREADS) void epipolar_decide_kernel(EpipolarArgs e)
{
    __shared__ unsigned long long wave_key[DECIDE_THREADS / 64];
    __shared__ double hyp_model[9], sums[45], final_model[9];
    __shared__ int final_valid, inlier_count;
    const ModelArgs &a = e.m;
    const ModelPair pr = pair_of<BATCH>(a);
    klt_epipolar_model *const record = reinterpret_cast<klt_epipolar_model *>(pr.model);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int m = *pr.count;
    const int size = (int)((unsigned)a.ncols | (unsigned)a.nrows << 16);
    const F9 none = {{0., 0., 0., 0., 0., 0., 0., 0., 0.}};
    if (m < a.min_inliers) {                                 // (uniform over the workgroup, like every return below)
        if (t == 0) write_model(record, none, 0, m, 0, -1, 0, size);
        return;
    }
    // the best hypothesis: the largest score, ties to the smallest h
    reduce_best_key<DECIDE_THREADS>(pr.scores, a.hypotheses, wave_key);
    if (t == 0) inlier_count = 0;
    __syncthreads();
    const unsigned long long key = best_key_of<DECIDE_THREADS>(wave_key);
    const int best_score = (int)(unsigned)(key >> 32) - 1;
    const int best = (int)(0xffffffffu - (unsigned)key);
    if (best_score < a.min_inliers) {
        if (t == 0) write_model(record, none, 0, m, 0, -1, 0, size);
        return;
    }
    if (w == 0) {
        F9 H;
        hypothesis(pr, a.seed, best, m, e.s, lane, H);       // (it scored: null9 succeeds again)
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) hyp_model[i] = H.f[i];
        }
    }
    __syncthreads();
    F9 H;
#pragma unroll
    for (int i = 0; i < 9; i++) H.f[i] = hyp_model[i];
    // M = SUM row^T row over its inliers: every wavefront adds its share of the 45 sums over ALL candidates
    static_assert(DECIDE_THREADS == 64 * 8, "one case per wavefront below");
    switch (w) {
    case 0: add_sums<0>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 1: add_sums<1>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 2: add_sums<2>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 3: add_sums<3>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 4: add_sums<4>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 5: add_sums<5>(pr, H, a.t2, e.s, m, lane, sums); break;
    case 6: add_sums<6>(pr, H, a.t2, e.s, m, lane, sums); break;
    default: add_sums<7>(pr, H, a.t2, e.s, m, lane, sums); break;
    }
    __syncthreads();
    if (w == 0) {
        // g: the largest |f_i| of the hypothesis, ties to the smallest i
        int g = 0;
        double big = fabs(H.f[0]);
#pragma unroll
        for (int i = 1; i < 9; i++) {
            const double v = fabs(H.f[i]);
            if (v > big) { big = v; g = i; }
        }
        // M without row g, one entry per lane: M[i][j], i <= j, is sum number 9 i - i (i - 1) / 2 + (j - i)
        const int row = (lane >> 3) + ((lane >> 3) >= g ? 1 : 0), col = lane & 7;
        const int lo = row < col ? row : col, hi = row < col ? col : row;
        const double ma = sums[9 * lo - ((lo * (lo - 1)) >> 1) + (hi - lo)];
        const double ma8 = sums[9 * row - ((row * (row - 1)) >> 1) + (8 - row)];
        F9 R;
        const bool refit = null9(ma, ma8, lane, R);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; i++) final_model[i] = refit ? R.f[i] : H.f[i];
            final_valid = refit ? 1 : 2;
        }
    }
    __syncthreads();
    F9 F;
#pragma unroll
    for (int i = 0; i < 9; i++) F.f[i] = final_model[i];
    int inliers = 0;
    for (int k0 = 0; k0 < m; k0 += DECIDE_THREADS * FINAL_AHEAD) {
        Cand cs[FINAL_AHEAD];
        bool ok[FINAL_AHEAD];
        load_working<FINAL_AHEAD>(pr.cand, k0 + t, DECIDE_THREADS, m, e.s, cs, ok);
#pragma unroll
        for (int j = 0; j < FINAL_AHEAD; j++) {
            const bool inl = ok[j] && is_inlier(F, a.t2, cs[j]);
            if (ok[j] && !inl) {
                const i32x2 id = *(reinterpret_cast<const i32x2 *>(pr.idx) + (k0 + t + DECIDE_THREADS * j));   // id.x < n: written by the gather
                const f32x4 rec = {-1.f, -1.f, __int_as_float(KLT_EPIPOLAR_OUTLIER), __int_as_float(id.y)};
                *reinterpret_cast<f32x4 *>(pr.out + id.x) = rec;
            }
            inliers += __popcll(__ballot(inl));
        }
    }
    if (lane == 0 && inliers) atomicAdd(&inlier_count, inliers);
    __syncthreads();
    if (t == 0) write_model(record, F, final_valid, m, inlier_count, best, best_score, size);
}

template <bool BATCH>
static void launch_all(hipStream_t s, const EpipolarArgs &e, int which)
{
    const unsigned pairs = BATCH ? (unsigned)e.m.npairs : 1u;
    if (which == 1)
        klt_launch((epipolar_score_kernel<BATCH>), dim3((e.m.hypotheses + SCORE_WAVES - 1) / SCORE_WAVES, pairs), dim3(64 * SCORE_WAVES), 0, s, e);
    if (which == 2) klt_launch((epipolar_decide_kernel<BATCH>), dim3(1, pairs), dim3(DECIDE_THREADS), 0, s, e);
}

}  // namespace epipolar_kernels

void launch_epipolar_score(hipStream_t s, const EpipolarArgs &e)
{
    if (e.m.pairs) epipolar_kernels::launch_all<true>(s, e, 1); else epipolar_kernels::launch_all<false>(s, e, 1);
}

void launch_epipolar_decide(hipStream_t s, const EpipolarArgs &e)
{
    if (e.m.pairs) epipolar_kernels::launch_all<true>(s, e, 2); else epipolar_kernels::launch_all<false>(s, e, 2);
}
