// Homography check (gfx950, wave64): klt_homography_check_async.  Three launches in stream order read two feature lists, find the frame
// pair's homography by a seeded consensus search over four-point hypotheses with one least-squares refit, and turn every tracked feature
// further than the threshold from where the homography sends it into (-1, -1, KLT_HOMOGRAPHY_OUTLIER, aux).  Nothing here reads a frame.
// THE RULE stands in include/klt_gpu.h ("homography check"), word for word what this file computes; DESIGN.md section 9i has it with its
// reasons, tests/homography_expected.py is its numpy restatement and the device equals that bit for bit.
//
// Everything is FP64 with one rounding per operation in the header's order, `+`, `-` and `*` only, no `/` or `%` by a run-time integer;
// every product and sum below is its own statement or parenthesis, and contraction is off.
//
//   (candidates)               model_gather_kernel of the motion-model check, unchanged, on this check's own scratch.
//   homography_score_kernel    one wavefront per hypothesis, four per workgroup.  The 8x9 matrix of the four picks (two rows each) lives
//                              in registers, one entry per lane, exactly as in epipolar_score_kernel, and goes through the same null9
//                              (consensus_primitives.h): no indexed private array, no scratch, no LDS, no barrier.  Then lanes stride over
//                              the candidates, four loaded ahead; one int32 score per hypothesis.
//   homography_decide_kernel   one workgroup of eight wavefronts per pair.  Argmax as in model_decide_kernel.  Wavefront 0 redoes the best
//                              hypothesis and hands it round through LDS; the eight wavefronts share the 24 sums of the structured normal
//                              matrix, three each, every one over all candidates -- lane l IS partial l of the rule --; wavefront 0 picks
//                              M without row g out of LDS, one entry per lane, runs null9 once more and publishes the final model; then
//                              all eight wavefronts test every candidate, scatter the outlier records (one 16-byte store each) and count;
//                              thread 0 writes the 96-byte model record.
// Batched form: blockIdx.y selects the pair from a table of ModelPair in device memory.
#include "consensus_primitives.h"

#pragma clang fp contract(off)

namespace homography_kernels {

using namespace consensus;

constexpr int SCORE_WAVES = 4;
constexpr int DECIDE_THREADS = 512;
constexpr int SCORE_AHEAD = 4, SUM_AHEAD = 8, FINAL_AHEAD = 4;      // candidates a lane loads before it uses the first

// step 5 of the rule: the forward transfer error, cross-multiplied
__device__ __forceinline__ bool is_inlier(const F9 &H, double t2, const Cand &c)
{
    const double *h = H.f;
    const double u0 = h[0] * c.px, u1 = h[1] * c.py, v0 = h[3] * c.px, v1 = h[4] * c.py, w0 = h[6] * c.px, w1 = h[7] * c.py;
    const double u = (u0 + u1) + h[2], v = (v0 + v1) + h[5], w = (w0 + w1) + h[8];
    const double wx = w * c.qx, wy = w * c.qy;
    const double rx = u - wx, ry = v - wy;
    const double r0 = rx * rx, r1 = ry * ry, ww = w * w;
    const double rr = r0 + r1, lim = t2 * ww;
    return rr <= lim;                                        // (NaN fails)
}

// entry `col` (0 .. 8) of row 2j + odd of correspondence c (step 3).  Every entry is +0.0, one of p.x, p.y, 1.0, or the negation of one
// product of q.x or q.y with p.x, p.y or 1.0; a product with 1.0 and a negation are exact.
__device__ __forceinline__ double row_entry(const Cand &c, bool odd, int col)
{
    const bool x = col == 0 || col == 3 || col == 6, y = col == 1 || col == 4 || col == 7;
    const double e = x ? c.px : (y ? c.py : 1.0);
    if (col < 6) return ((col >= 3) == odd) ? e : 0.0;
    const double q = odd ? c.qy : c.qx;
    const double t = q * e;
    return -t;
}

// steps 2 to 4 for hypothesis h: the eight rows of its four picks, one entry per lane, and their null vector
__device__ __forceinline__ bool hypothesis(const ModelPair &pr, uint32_t seed, int h, int m, double s, int lane, F9 &H)
{
    const Cand c = working(load_cand(pr.cand, pick<4>(seed, (uint32_t)h, (uint32_t)(lane >> 4), m)), s);
    const bool odd = ((lane >> 3) & 1) != 0;
    return null9(row_entry(c, odd, lane & 7), row_entry(c, odd, 8), lane, H);
}

template <bool BATCH>
__global__ __launch_bounds__(64 * SCORE_WAVES) void homography_score_kernel(EpipolarArgs e)
{
    const ModelArgs &a = e.m;
    const ModelPair pr = pair_of<BATCH>(a);
    const int lane = threadIdx.x & 63;
    const int h = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SCORE_WAVES + (threadIdx.x >> 6)));
    if (h >= a.hypotheses) return;
    const int m = *pr.count;
    if (m < a.min_inliers) return;                           // no model: the decision does not look at the scores
    F9 H;
    int score = -1;
    if (hypothesis(pr, a.seed, h, m, e.s, lane, H)) {
        score = 0;
        for (int k0 = 0; k0 < m; k0 += 64 * SCORE_AHEAD) {  // (a count: the order of the candidates does not matter)
            Cand c[SCORE_AHEAD];
            bool ok[SCORE_AHEAD];
            load_working<SCORE_AHEAD>(pr.cand, k0 + lane, 64, m, e.s, c, ok);
#pragma unroll
            for (int j = 0; j < SCORE_AHEAD; j++) score += __popcll(__ballot(ok[j] && is_inlier(H, a.t2, c[j])));
        }
    }
    if (lane == 0) pr.scores[h] = score;
}

__device__ __forceinline__ void write_model(klt_homography_model *dst, const F9 &H, int valid, int m, int n_inliers, int hyp, int hyp_inliers,
                                            int size)
{
    klt_homography_model r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.h[i] = H.f[i];
    r.valid = valid; r.n_candidates = m; r.n_inliers = n_inliers; r.hypothesis = hyp; r.hypothesis_inliers = hyp_inliers; r.pad = size;
    *dst = r;
}

// The sums number W, W + 8, W + 16 of the 24 (sum 6 b + t: block b = 0 A, 1 Bx, 2 By, 3 C; t = 0 .. 5 the pair (i, j), i <= j, of
// e = (p.x, p.y, 1) in the order 00 01 02 11 12 22) over the inliers of H, added by ONE wavefront over all candidates -- lane l is
// partial l of the rule, candidates l, l + 64, ... in increasing k --, folded, into sums[].  Each sum is added exactly as the rule says.
template <int W>
__device__ __forceinline__ void add_sums(const ModelPair &pr, const F9 &H, double t2, double s, int m, int lane, double *sums)
{
    double S[3] = {0., 0., 0.};
    for (int k0 = 0; k0 < m; k0 += 64 * SUM_AHEAD) {
        Cand cs[SUM_AHEAD];
        bool ok[SUM_AHEAD];
        load_working<SUM_AHEAD>(pr.cand, k0 + lane, 64, m, s, cs, ok);
#pragma unroll
        for (int j = 0; j < SUM_AHEAD; j++) {
            const Cand c = cs[j];
            if (ok[j] && is_inlier(H, t2, c)) {
                const double e[3] = {c.px, c.py, 1.0};
                const double qx2 = c.qx * c.qx, qy2 = c.qy * c.qy;
                const double qq = qx2 + qy2;
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const int u = W + 8 * q, b = u / 6, t = u % 6;                  // (compile-time constants after unrolling)
                    const int ti = t < 3 ? 0 : (t < 5 ? 1 : 2), tj = t < 3 ? t : (t < 5 ? t - 2 : 2);
                    const double ee = e[ti] * e[tj];
                    const double term = b == 0 ? ee : (b == 1 ? c.qx * ee : (b == 2 ? c.qy * ee : qq * ee));
                    S[q] = S[q] + term;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const double f = fold64(S[q]);
        if (lane == 0) sums[W + 8 * q] = f;
    }
}

// entry (row, col) of M = [[A, 0, -Bx], [0, A, -By], [-Bx, -By, C]] out of the 24 sums
__device__ __forceinline__ double normal_entry(const double *sums, int row, int col)
{
    const int bi = row / 3, bj = col / 3;                    // (constant divisors: multiplications)
    const int i = row - 3 * bi, j = col - 3 * bj;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int t = 3 * lo - ((lo * (lo - 1)) >> 1) + (hi - lo);
    if (bi == bj) return sums[(bi == 2 ? 18 : 0) + t];
    if (bi != 2 && bj != 2) return 0.0;
    const int other = bi < bj ? bi : bj;
    return -sums[6 + 6 * other + t];
}

template <bool BATCH>
__global__ __launch_bounds__(DECIDE_THREADS) void homography_decide_kernel(EpipolarArgs e)
{
    __shared__ unsigned long long wave_key[DECIDE_THREADS / 64];
    __shared__ double hyp_model[9], sums[24], final_model[9];
    __shared__ int final_valid, inlier_count;
    const ModelArgs &a = e.m;
    const ModelPair pr = pair_of<BATCH>(a);
    klt_homography_model *const record = reinterpret_cast<klt_homography_model *>(pr.model);
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
    // the 24 sums of M over its inliers: every wavefront adds its three over ALL candidates
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
        // g: the largest |h_i| of the hypothesis, ties to the smallest i
        int g = 0;
        double big = fabs(H.f[0]);
#pragma unroll
        for (int i = 1; i < 9; i++) {
            const double v = fabs(H.f[i]);
            if (v > big) { big = v; g = i; }
        }
        // M without row g, one entry per lane
        const int row = (lane >> 3) + ((lane >> 3) >= g ? 1 : 0);
        const double ma = normal_entry(sums, row, lane & 7);
        const double ma8 = normal_entry(sums, row, 8);
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
                const f32x4 rec = {-1.f, -1.f, __int_as_float(KLT_HOMOGRAPHY_OUTLIER), __int_as_float(id.y)};
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
        klt_launch((homography_score_kernel<BATCH>), dim3((e.m.hypotheses + SCORE_WAVES - 1) / SCORE_WAVES, pairs), dim3(64 * SCORE_WAVES), 0, s, e);
    if (which == 2) klt_launch((homography_decide_kernel<BATCH>), dim3(1, pairs), dim3(DECIDE_THREADS), 0, s, e);
}

}  // namespace homography_kernels

void launch_homography_score(hipStream_t s, const EpipolarArgs &e)
{
    if (e.m.pairs) homography_kernels::launch_all<true>(s, e, 1); else homography_kernels::launch_all<false>(s, e, 1);
}

void launch_homography_decide(hipStream_t s, const EpipolarArgs &e)
{
    if (e.m.pairs) homography_kernels::launch_all<true>(s, e, 2); else homography_kernels::launch_all<false>(s, e, 2);
}
