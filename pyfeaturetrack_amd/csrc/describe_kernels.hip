// Binary descriptors (gfx950): klt_describe_async.  The rule stands in include/klt_gpu.h ("descriptors"), the pattern and the cosine table
// in describe_rule.h; DESIGN.md section 9n.  Integer arithmetic throughout: the records equal tests/describe_expected.py byte for byte.
//
//   describe_kernel<STEERED>   one wavefront per feature, four per workgroup.  The in-frame part of the 31 x 31 patch around the centre is
//                              staged into LDS in 4-byte pieces cut on the ADDRESS (a piece inside the row is one aligned dword load
//                              whatever the centre and the frame's width, the ragged ends come byte by byte; nothing outside the rows'
//                              in-frame bytes is touched), the replicated edge is a clamp of the LDS index.  The 5 x 5 box sums are
//                              formed separably in LDS as 16-bit sums (at most 6375); the steered form takes the two moments of the disc
//                              by a wave reduction and the 32 scores in 64-bit integers.  Lane L then evaluates tests L, L + 64, L + 128,
//                              L + 192: each 64-bit ballot is two finished words of the record, which lanes 0 .. 2 store as three
//                              16-byte pieces.  The pattern comes from device memory (1 KB) into LDS once per workgroup.
#include "klt_internal.h"
#include "describe_rule.h"

namespace describe_kernels {

using namespace kltapi;

constexpr int WAVES = 4;
constexpr int SIDE = 2 * kDescDisc + 1;           // 31: the patch
constexpr int PITCH = 32;                         // bytes from row to row of the patch in LDS
constexpr int SUMS = 2 * kDescReach + 1;          // 27: box centres per axis
constexpr int SPITCH = 28;                        // 16-bit sums from row to row

template <bool STEERED>
__global__ __launch_bounds__(WAVES * 64) void describe_kernel(DescribeArgs a)
{
    __shared__ uint32_t pat[kDescTests];
    __shared__ uint8_t patch_all[WAVES][SIDE * PITCH];
    __shared__ uint16_t hsum_all[WAVES][SIDE * SPITCH];
    __shared__ uint16_t box_all[WAVES][SUMS * SPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * WAVES + wave;
    uint8_t *patch = patch_all[wave];
    uint16_t *hsum = hsum_all[wave], *box = box_all[wave];
    pat[tid] = reinterpret_cast<const uint32_t *>(a.pattern)[tid];      // (kDescTests == WAVES * 64)

    // the centre: every lane of the wavefront looks at the same record
    bool work = false;
    int cx = 0, cy = 0;
    if (i < a.n) {
        const klt_feat f = a.in[i];
        if (f.val >= 0 && isfinite(f.x) && isfinite(f.y)) {
            const double fx = floor((double)f.x + 0.5), fy = floor((double)f.y + 0.5);
            if (fx >= 0.0 && fx < (double)a.ncols && fy >= 0.0 && fy < (double)a.nrows) {
                work = true;
                cx = (int)fx; cy = (int)fy;
            }
        }
    }
    const int ox = cx - kDescDisc, oy = cy - kDescDisc;      // frame position of the patch's corner
    if (work) {
        const int xa = ox < 0 ? 0 : ox, xb = cx + kDescDisc > a.ncols - 1 ? a.ncols - 1 : cx + kDescDisc;
        const int ya = oy < 0 ? 0 : oy, yb = cy + kDescDisc > a.nrows - 1 ? a.nrows - 1 : cy + kDescDisc;
        const int w = xb - xa + 1, h = yb - ya + 1;
        const int per_row = (w + 6) >> 2;                    // a row segment that starts up to 3 bytes into a piece touches at most this many
        for (int it = lane; it < per_row * h; it += 64) {
            const int r = it / per_row, c = it - r * per_row;
            const uint8_t *row = a.frame + (size_t)(ya + r) * (size_t)a.ncols + xa;
            const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
            const int first = 4 * c - mis;                   // the piece's first byte, relative to the row segment
            const int lo = first < 0 ? -first : 0, hi = w - first < 4 ? w - first : 4;
            if (hi <= lo) continue;
            uint8_t *dst = patch + (ya + r - oy) * PITCH + (xa + first - ox);
            if (lo == 0 && hi == 4) {
                const uint32_t q = *reinterpret_cast<const uint32_t *>(row + first);
                dst[0] = (uint8_t)q; dst[1] = (uint8_t)(q >> 8); dst[2] = (uint8_t)(q >> 16); dst[3] = (uint8_t)(q >> 24);
            } else {
                for (int k = lo; k < hi; k++) dst[k] = row[first + k];
            }
        }
    }
    __syncthreads();

    // P(u, v) with the replicated edge: the clamp of the frame position, taken on the LDS index
    auto P = [&](int u, int v) -> int {
        int x = cx + u, y = cy + v;
        x = x < 0 ? 0 : x > a.ncols - 1 ? a.ncols - 1 : x;
        y = y < 0 ? 0 : y > a.nrows - 1 ? a.nrows - 1 : y;
        return patch[(y - oy) * PITCH + (x - ox)];
    };
    int k = 0;
    if (work) {
        for (int it = lane; it < SIDE * SUMS; it += 64) {    // horizontal sums of five: rows -15 .. 15, centres -13 .. 13
            const int r = it / SUMS, c = it - r * SUMS;
            const int v = r - kDescDisc, u = c - kDescReach;
            hsum[r * SPITCH + c] = (uint16_t)(P(u - 2, v) + P(u - 1, v) + P(u, v) + P(u + 1, v) + P(u + 2, v));
        }
        if constexpr (STEERED) {
            int m10 = 0, m01 = 0;                            // (at most 15 * 255 * 709 in magnitude: 32 bits hold them)
            for (int it = lane; it < SIDE * SIDE; it += 64) {
                const int r = it / SIDE, c = it - r * SIDE;
                const int v = r - kDescDisc, u = c - kDescDisc;
                if (u * u + v * v <= kDescDisc * kDescDisc) {
                    const int p = P(u, v);
                    m10 += u * p; m01 += v * p;
                }
            }
            for (int m = 32; m >= 1; m >>= 1) { m10 += __shfl_xor(m10, m); m01 += __shfl_xor(m01, m); }
            long long best = 0;
#pragma unroll
            for (int j = 0; j < kDescBins; j++) {
                const long long sc = (long long)m10 * (long long)a.cs[j] + (long long)m01 * (long long)a.cs[(j + 24) & 31];
                if (j == 0 || sc > best) { best = sc; k = j; }
            }
        }
    }
    __syncthreads();
    if (work) {
        for (int it = lane; it < SUMS * SUMS; it += 64) {    // vertical sums of five: the boxes centred at -13 .. 13 on both axes
            const int r = it / SUMS, c = it - r * SUMS;
            const uint16_t *p = hsum + (r + kDescBox) * SPITCH + c;      // (row r + 2 of hsum is v = r - 13)
            box[r * SPITCH + c] = (uint16_t)(p[-2 * SPITCH] + p[-SPITCH] + p[0] + p[SPITCH] + p[2 * SPITCH]);
        }
    }
    __syncthreads();
    if (i >= a.n) return;

    unsigned long long words[4] = {0ull, 0ull, 0ull, 0ull};
    if (work) {
        const int ck = a.cs[k], sk = a.cs[(k + 24) & 31];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t t = pat[lane + 64 * j];
            int ax = (int8_t)(t & 0xff), ay = (int8_t)((t >> 8) & 0xff), bx = (int8_t)((t >> 16) & 0xff), by = (int8_t)(t >> 24);
            if (STEERED && k != 0) {
                const int rax = (ax * ck - ay * sk + 8192) >> 14, ray = (ax * sk + ay * ck + 8192) >> 14;
                const int rbx = (bx * ck - by * sk + 8192) >> 14, rby = (bx * sk + by * ck + 8192) >> 14;
                ax = rax; ay = ray; bx = rbx; by = rby;
            }
            const int sa = box[(ay + kDescReach) * SPITCH + ax + kDescReach], sb = box[(by + kDescReach) * SPITCH + bx + kDescReach];
            words[j] = __ballot(sa < sb);
        }
    }
    if (lane < 3) {
        uint4 piece;
        if (lane < 2) {
            const unsigned long long w0 = lane == 0 ? words[0] : words[2], w1 = lane == 0 ? words[1] : words[3];
            piece = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            piece = work ? make_uint4(1u, (uint32_t)k, (uint32_t)cx, (uint32_t)cy) : make_uint4(0u, 0u, 0u, 0u);
        }
        reinterpret_cast<uint4 *>(a.out + i)[lane] = piece;
    }
}

}  // namespace describe_kernels

void launch_describe(hipStream_t s, const DescribeArgs &a, int mode)
{
    using namespace describe_kernels;
    const dim3 grid((unsigned)((a.n + WAVES - 1) / WAVES)), block(WAVES * 64);
    if (mode == 2) klt_launch(describe_kernel<true>, grid, block, 0, s, a);
    else klt_launch(describe_kernel<false>, grid, block, 0, s, a);
}
