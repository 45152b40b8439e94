// remap_kernels.hip -- the remap ingest stage: a fixed-point remap with bilinear interpolation of 8-bit frames in front of the level-0
// kernel (not in the reference).  The rule stands in include/klt_gpu.h: integer arithmetic only, so that the bytes
// are those of the numpy restatement (tests/remap_expected.py).  One launch for up to KLT_MAX_BATCH frames of one size under one map:
//   remap_kernel   A lane owns 4 consecutive destination pixels of one row, a piece cut on the destination's ADDRESS: a piece inside the
//                  row is one aligned dword store and -- the map's planes are laid out like the destination, 4 bytes an entry -- two
//                  aligned dwordx4 loads of map entries; the pieces at the two ragged ends of a row read their entries one by one and
//                  store single bytes, never past the row.  A wavefront takes a tile of 64 x 4 destination pixels (16 pieces across, 4
//                  rows down), a workgroup four such tiles one below the other: under a rotation-like map a wavefront's source footprint
//                  is a compact patch, not a long diagonal.  Every entry is clamped here, whatever the host sent: no map content makes
//                  an address outside the source rows.  The lane turns its entries into a source offset and a packed weight word ONCE
//                  and then walks the frames of the batch (the map is 8 bytes a pixel, a frame 1 read and 1 written: the map is read
//                  once per launch, not once per frame); the four source bytes of a pixel are gathered as two 2-byte loads, one per
//                  source row (byte loads in a frame one pixel wide).
// Plain C++ and vector memory operations only; no LDS, no scratch.
#include "klt_internal.h"

namespace remap_kernels {

constexpr int THREADS = 256;
constexpr int PIECE = 4;                 // destination pixels per lane
constexpr int PIECES_ACROSS = 16;        // pieces of a row per wavefront: 64 pixels
constexpr int WAVE_ROWS = 4, GROUP_ROWS = 16;

// one map entry -> where the four source pixels are and what they weigh.  `w`: fx | fy << 8 | (x1 - x0) << 16 | (y1 - y0) << 17.
// `off`: a byte offset in the source frame (below 2^28: the host's shape test) -- of p00, or, PAIRS (frames two or more pixels wide:
// the two pixels of a row come as one 2-byte load), of the pair's first byte: p00 where x1 = x0 + 1, the pixel left of it where
// x0 is the row's last pixel (x1 = x0, fx = 0), so that no pair reaches past its row
template <bool PAIRS>
__device__ inline void place(int mx, int my, const RemapArgs &a, unsigned &off, unsigned &w)
{
    const int X = min(max(mx, 0), (a.ncols - 1) << 8), Y = min(max(my, 0), (a.nrows - 1) << 8);      // (ncols, nrows <= 65535: below 2^24)
    const int x0 = X >> 8, y0 = Y >> 8;
    const unsigned right = x0 + 1 < a.ncols ? 1u : 0u, down = y0 + 1 < a.nrows ? 1u : 0u;            // x1 = min(x0 + 1, ncols - 1), y1 likewise
    off = (unsigned)y0 * (unsigned)a.src_pitch + (unsigned)x0 - (PAIRS ? 1u - right : 0u);           // (PAIRS: ncols >= 2, so x0 >= 1 where right is 0)
    w = (unsigned)(X & 255) | (unsigned)(Y & 255) << 8 | right << 16 | down << 17;
}

// two neighbouring bytes of a row, the first in the low half (no alignment is promised: the compiler picks a load the target allows)
__device__ inline unsigned pair_at(const uint8_t *p)
{
    unsigned short v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

template <bool PAIRS>
__device__ inline unsigned sample(const uint8_t *src, unsigned off, unsigned w, unsigned pitch)
{
    const unsigned fx = w & 255u, fy = (w >> 8) & 255u, right = (w >> 16) & 1u, down = (w >> 17) & 1u ? pitch : 0u;
    const uint8_t *p = src + off;
    unsigned p00, p10, p01, p11;
    if (PAIRS) {
        const unsigned top = pair_at(p), bottom = pair_at(p + down);
        p10 = top >> 8; p11 = bottom >> 8;                       // (x1's pixel is the pair's second byte either way)
        p00 = right ? top & 255u : p10; p01 = right ? bottom & 255u : p11;
    } else {
        p00 = p[0]; p10 = p[right]; p01 = p[down]; p11 = p[down + right];
    }
    // (at most 65536 * 255 + 32768: unsigned 32 bits hold it)
    return ((256u - fx) * (256u - fy) * p00 + fx * (256u - fy) * p10 + (256u - fx) * fy * p01 + fx * fy * p11 + 32768u) >> 16;
}

template <bool PAIRS>
__global__ __launch_bounds__(THREADS) void remap_kernel(RemapArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = (int)blockIdx.y * GROUP_ROWS + wave * WAVE_ROWS + (lane >> 4);
    if (y >= a.nrows) return;
    // the destinations are ncols bytes from row to row behind a 16-byte aligned base (so are the map's planes, 4 bytes an entry): the
    // row's pieces are cut where its index, counted from the frame's first pixel, is a multiple of 4
    const size_t row = (size_t)y * (size_t)a.ncols;
    const int first = PIECE * ((int)blockIdx.x * PIECES_ACROSS + (lane & 15)) - (int)(row & 3);      // the piece's first pixel in the row
    const int lo = first < 0 ? -first : 0, hi = a.ncols - first < PIECE ? a.ncols - first : PIECE;
    if (hi <= lo) return;
    const size_t at = row + first;                           // (first >= -(row & 3): not below the row's own piece)
    const bool whole = lo == 0 && hi == PIECE;
    unsigned off[PIECE], w[PIECE];
    if (whole) {
        const int4 qx = *reinterpret_cast<const int4 *>(a.map_x + at), qy = *reinterpret_cast<const int4 *>(a.map_y + at);
        place<PAIRS>(qx.x, qy.x, a, off[0], w[0]);
        place<PAIRS>(qx.y, qy.y, a, off[1], w[1]);
        place<PAIRS>(qx.z, qy.z, a, off[2], w[2]);
        place<PAIRS>(qx.w, qy.w, a, off[3], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < PIECE; k++) {
            off[k] = w[k] = 0;
            if (k >= lo && k < hi) place<PAIRS>(a.map_x[at + k], a.map_y[at + k], a, off[k], w[k]);
        }
    }
    const unsigned pitch = (unsigned)a.src_pitch;
    for (int b = 0; b < a.batch; b++) {
        const uint8_t *src = a.src[b];
        uint8_t *dst = a.dst[b] + at;
        if (whole) {
            unsigned out = 0;
#pragma unroll
            for (int k = 0; k < PIECE; k++) out |= sample<PAIRS>(src, off[k], w[k], pitch) << (8 * k);
            *reinterpret_cast<unsigned *>(dst) = out;        // (4-byte aligned: the cut)
        } else {
#pragma unroll
            for (int k = 0; k < PIECE; k++)
                if (k >= lo && k < hi) dst[k] = (uint8_t)sample<PAIRS>(src, off[k], w[k], pitch);
        }
    }
}

}  // namespace remap_kernels

void launch_remap(hipStream_t s, const RemapArgs &a)
{
    using namespace remap_kernels;
    // a row of ncols bytes that starts up to 3 bytes into an aligned piece touches at most (ncols + 6) / 4 of them
    const int per_row = (a.ncols + 2 * (PIECE - 1)) / PIECE;
    const dim3 grid((unsigned)((per_row + PIECES_ACROSS - 1) / PIECES_ACROSS), (unsigned)((a.nrows + GROUP_ROWS - 1) / GROUP_ROWS));
    if (a.ncols >= 2) klt_launch(remap_kernel<true>, grid, dim3(THREADS), 0, s, a);
    else klt_launch(remap_kernel<false>, grid, dim3(THREADS), 0, s, a);      // (a frame one pixel wide has no pairs)
}
