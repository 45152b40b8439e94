// equalize_kernels.hip -- contrast-limited adaptive histogram equalisation (CLAHE) of 8-bit frames in front of the level-0 kernel (not in
// the reference).  The rule stands in include/klt_gpu.h: integer arithmetic only, so that the bytes are those of
// the numpy restatement (tests/equalize_expected.py).  Two launches, up to KLT_MAX_BATCH frames of one size in each (blockIdx.y):
//   clahe_lut_kernel    ONE workgroup of 1024 lanes per (tile, frame).  The tile's rows are read in 16-byte pieces cut on the ADDRESS (so a
//                       piece inside the row is one aligned dwordx4 load whatever the pitch; the pieces at the two ragged ends are read
//                       byte by byte and never past the row), a lane merges the equal neighbours of its piece before it adds (a constant
//                       tile: one ds_add per 16 pixels, not sixteen on one bin), and the adds of a workgroup are spread over 16 copies of
//                       the histogram in LDS (lanes that share a copy are 16 apart).  Then one lane per bin: sum of the copies, clip,
//                       redistribute, an inclusive scan over the 256 bins in LDS, the 64-bit product divided in 8 steps of long division (every
//                       division of the file is a full 32-bit one: no expansion with a fused multiply-add), one LUT byte out.
//   clahe_apply_kernel  the frame is cut into the (tiles_y + 1) bands of rows between the tile centres: all pixels of a band interpolate
//                       between the same two LUT rows, which a workgroup holds in LDS (2 * tiles_x * 256 bytes, at most 32 KB) beside the
//                       table of the column centres.  A band is split over `split` workgroups; a lane takes 16 output pixels at a time
//                       (pieces cut on the destination's address: aligned dwordx4 stores inside the row, bytes at the ragged ends; the
//                       16 source bytes come as one dwordx4 load when their address is aligned too, which is so for every frame a slot
//                       holds), walks the column centres along the piece, and does the four products and one 32-bit division per pixel.
// Plain C++ and vector memory operations only.
#include "klt_internal.h"

namespace equalize_kernels {

constexpr int LUT_THREADS = 1024;
constexpr int HIST_COPIES = 16;
constexpr int APPLY_THREADS = 256;

// every division of the two kernels is a 32-bit one (k <= 65, n <= 65535, tiles <= 64: k * n fits)
__device__ inline int tile_edge(int k, int n, int tiles) { return (int)(((unsigned)k * (unsigned)n) / (unsigned)tiles); }

// the bytes [lo, hi) of a row piece of 16 (`lo`, `hi` in 0 .. 16, relative to the piece's first byte, which is p): a whole aligned piece as
// one load, anything else byte by byte
__device__ inline void load_piece(const uint8_t *p, int lo, int hi, uint8_t v[16])
{
    if (lo == 0 && hi == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = (i >= lo && i < hi) ? p[i] : (uint8_t)0;
    }
}

__global__ __launch_bounds__(LUT_THREADS) void clahe_lut_kernel(EqualizeArgs a)
{
    __shared__ unsigned hist[HIST_COPIES * 256];
    __shared__ unsigned scan[2][256];
    __shared__ unsigned excess_sum;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const uint8_t *src = a.src[blockIdx.y];
    const int x0 = tile_edge(tx, a.ncols, a.tiles_x), x1 = tile_edge(tx + 1, a.ncols, a.tiles_x);
    const int y0 = tile_edge(ty, a.nrows, a.tiles_y), y1 = tile_edge(ty + 1, a.nrows, a.tiles_y);
    const int w = x1 - x0, h = y1 - y0;
    for (int i = tid; i < HIST_COPIES * 256; i += LUT_THREADS) hist[i] = 0;
    if (tid == 0) excess_sum = 0;
    __syncthreads();

    // pieces per row: a row segment of w bytes that starts up to 15 bytes into an aligned piece touches at most (w + 30) / 16 of them
    unsigned *mine = hist + (tid & (HIST_COPIES - 1)) * 256;
    const int per_row = (w + 30) >> 4, items = per_row * h;
    for (int it = tid; it < items; it += LUT_THREADS) {
        const int r = (int)((unsigned)it / (unsigned)per_row), c = it - r * per_row;
        const uint8_t *row = src + (size_t)(y0 + r) * a.src_pitch + x0;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int first = 16 * c - mis;                      // the piece's first byte, relative to the row segment
        int lo = first < 0 ? -first : 0, hi = w - first < 16 ? w - first : 16;
        if (hi <= lo) continue;                              // (the last counted piece of a row that needed one fewer)
        uint8_t v[16];
        load_piece(row + first, lo, hi, v);
        // equal neighbours merged: one add per run
        unsigned run = 0, cur = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i < lo || i >= hi) continue;
            if (run && v[i] == cur) { run++; continue; }
            if (run) atomicAdd(&mine[cur], run);
            cur = v[i];
            run = 1;
        }
        atomicAdd(&mine[cur], run);                          // (hi > lo: the piece holds a pixel)
    }
    __syncthreads();

    const unsigned A = (unsigned)w * (unsigned)h;
    unsigned hb = 0, over = 0, cap = 0;
    if (tid < 256) {
#pragma unroll
        for (int k = 0; k < HIST_COPIES; k++) hb += hist[k * 256 + tid];
        if (a.clip_q8 > 0) {
            const unsigned long long q = ((unsigned long long)a.clip_q8 * A) >> 16;
            cap = q < 1 ? 1u : (unsigned)q;                  // (q <= 2^20 * 2^27 >> 16 = 2^31)
            over = hb > cap ? hb - cap : 0;
        }
    }
    if (a.clip_q8 > 0) {
        // the excess of the 256 bins: wave sums in registers, one add per wave
        if (tid < 256) {
            unsigned s = over;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
            if ((tid & 63) == 0) atomicAdd(&excess_sum, s);
        }
        __syncthreads();
        if (tid < 256) {
            const unsigned excess = excess_sum, r = excess & 255u;
            hb = (hb > cap ? cap : hb) + (excess >> 8);
            // bins (k * 256) / r, k = 0 .. r - 1, get one more each.  Bin b is hit iff some k has b <= k * 256 / r < b + 1, i.e. iff the
            // smallest k with k * 256 >= b * r also has k * 256 < (b + 1) * r (which is at most 256 * r, so that k is below r); r < 256,
            // so no bin is hit twice
            const unsigned k = ((unsigned)tid * r + 255u) >> 8;
            if (k * 256u < ((unsigned)tid + 1u) * r) hb++;
        }
    }
    // inclusive scan over the bins (Hillis-Steele, two buffers)
    if (tid < 256) scan[0][tid] = hb;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < 256; d <<= 1) {
        if (tid < 256) scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    if (tid < 256) {
        // (cdf * 255 + A / 2) / A: a 64-bit numerator (cdf <= A < 2^27), a quotient of 8 bits -- long division, one bit per step
        unsigned long long num = (unsigned long long)scan[cur][tid] * 255ull + (A >> 1);
        unsigned q = 0;
#pragma unroll
        for (int bit = 7; bit >= 0; bit--) {
            const unsigned long long d = (unsigned long long)A << bit;
            if (num >= d) { num -= d; q |= 1u << bit; }
        }
        a.lut[blockIdx.y][(size_t)tile * 256 + tid] = (uint8_t)q;
    }
}

// centre of tile k in doubled coordinates: x_k + x_{k+1}
__device__ inline int tile_centre(int k, int n, int tiles) { return tile_edge(k, n, tiles) + tile_edge(k + 1, n, tiles); }

__global__ __launch_bounds__(APPLY_THREADS) void clahe_apply_kernel(EqualizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint8_t *lut_top = smem, *lut_bot = smem + a.tiles_x * 256;
    int *centre = reinterpret_cast<int *>(smem + 2 * a.tiles_x * 256);      // [tiles_x]
    const int tid = threadIdx.x;
    const int band = (int)(blockIdx.x / (unsigned)a.split), part = (int)blockIdx.x - band * a.split;      // band j: rows with C_{j-1} <= 2y + 1 < C_j
    const uint8_t *src = a.src[blockIdx.y];
    uint8_t *dst = a.dst[blockIdx.y];
    const int Ty = a.tiles_y, Tx = a.tiles_x;
    const int c_above = band >= 1 ? tile_centre(band - 1, a.nrows, Ty) : 0, c_below = band < Ty ? tile_centre(band, a.nrows, Ty) : 0;
    const int band_y0 = band >= 1 ? c_above >> 1 : 0, band_y1 = band < Ty ? c_below >> 1 : a.nrows;      // 2y + 1 >= C  <=>  y >= C >> 1
    const int rows = band_y1 - band_y0;
    const int ya = band_y0 + (int)(((unsigned)rows * (unsigned)part) / (unsigned)a.split);            // (rows <= 65535, split <= 1024)
    const int yb = band_y0 + (int)(((unsigned)rows * (unsigned)(part + 1)) / (unsigned)a.split);
    if (ya >= yb) return;                                    // (workgroup-uniform: before any barrier)
    const bool inner_y = band >= 1 && band < Ty;
    const int t_top = band >= 1 ? band - 1 : 0, t_bot = band < Ty ? band : Ty - 1;
    const unsigned Dy = inner_y ? (unsigned)(c_below - c_above) : 1u;
    {
        const uint4 *gt = reinterpret_cast<const uint4 *>(a.lut[blockIdx.y] + (size_t)t_top * Tx * 256);
        const uint4 *gb = reinterpret_cast<const uint4 *>(a.lut[blockIdx.y] + (size_t)t_bot * Tx * 256);
        for (int i = tid; i < Tx * 16; i += APPLY_THREADS) {
            reinterpret_cast<uint4 *>(lut_top)[i] = gt[i];
            reinterpret_cast<uint4 *>(lut_bot)[i] = gb[i];
        }
        for (int k = tid; k < Tx; k += APPLY_THREADS) centre[k] = tile_centre(k, a.ncols, Tx);
    }
    __syncthreads();

    const int nc = a.ncols;
    const int per_row = (nc + 30) >> 4, items = per_row * (yb - ya);
    for (int it = tid; it < items; it += APPLY_THREADS) {
        const int r = (int)((unsigned)it / (unsigned)per_row), c = it - r * per_row;
        const int y = ya + r;
        uint8_t *drow = dst + (size_t)y * nc;
        const uint8_t *srow = src + (size_t)y * a.src_pitch;
        const int mis = (int)(reinterpret_cast<uintptr_t>(drow) & 15);
        const int first = 16 * c - mis;
        const int lo = first < 0 ? -first : 0, hi = nc - first < 16 ? nc - first : 16;
        if (hi <= lo) continue;
        uint8_t v[16];
        load_piece(srow + first, lo, hi, v);
        const unsigned wy = inner_y ? (unsigned)(2 * y + 1 - c_above) : 0u;
        // the number of column centres at or left of the piece's first pixel: from the tile that holds it, then walked along the piece
        const int xs = first + lo;
        const int t = (int)((((unsigned)xs + 1u) * (unsigned)Tx - 1u) / (unsigned)nc);
        int i = t + (2 * xs + 1 >= centre[t] ? 1 : 0);
        unsigned out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < lo || k >= hi) continue;
            const int P = 2 * (first + k) + 1;
            if (i < Tx && P >= centre[i]) i++;               // (centres are at least 2 apart: one step per pixel at most)
            const bool inner_x = i >= 1 && i < Tx;
            const int tl = i >= 1 ? i - 1 : 0, tr = i < Tx ? i : Tx - 1;
            const unsigned wx = inner_x ? (unsigned)(P - centre[i - 1]) : 0u;
            const unsigned Dx = inner_x ? (unsigned)(centre[i] - centre[i - 1]) : 1u;
            const unsigned l00 = lut_top[tl * 256 + v[k]], l10 = lut_top[tr * 256 + v[k]];
            const unsigned l01 = lut_bot[tl * 256 + v[k]], l11 = lut_bot[tr * 256 + v[k]];
            const unsigned D = Dx * Dy;                      // (D * 255 < 2^32: the host's shape test)
            const unsigned sum = l00 * (Dx - wx) * (Dy - wy) + l10 * wx * (Dy - wy) + l01 * (Dx - wx) * wy + l11 * wx * wy;
            // (sum + D / 2) / D without the sum that could pass 2^32: the quotient, one more when the remainder reaches D - D / 2
            const unsigned q = sum / D;
            out[k >> 2] |= (q + ((sum - q * D) + (D >> 1) >= D ? 1u : 0u)) << (8 * (k & 3));
        }
        if (lo == 0 && hi == 16) {
            *reinterpret_cast<uint4 *>(drow + first) = make_uint4(out[0], out[1], out[2], out[3]);      // (drow + first is 16-byte aligned)
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k >= lo && k < hi) drow[first + k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
        }
    }
}

}  // namespace equalize_kernels

size_t equalize_apply_lds_bytes(int tiles_x) { return (size_t)2 * tiles_x * 256 + (((size_t)tiles_x * sizeof(int) + 15) & ~(size_t)15); }

void launch_clahe_lut(hipStream_t s, const EqualizeArgs &a, int batch)
{
    klt_launch(equalize_kernels::clahe_lut_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)batch), dim3(equalize_kernels::LUT_THREADS), 0, s, a);
}

void launch_clahe_apply(hipStream_t s, const EqualizeArgs &a, int batch)
{
    klt_launch(equalize_kernels::clahe_apply_kernel, dim3((unsigned)((a.tiles_y + 1) * a.split), (unsigned)batch),
               dim3(equalize_kernels::APPLY_THREADS), (unsigned)equalize_apply_lds_bytes(a.tiles_x), s, a);
}
