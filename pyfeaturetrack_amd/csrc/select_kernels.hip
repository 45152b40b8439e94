// Corner selection on gfx950: summed-area tables, min-eigenvalue score, candidate sort, greedy
// minimum-distance suppression.
//
// Parity notes:
//   * numpy's `cumsum(1).cumsum(0)` on f32 is a strictly sequential f32 prefix per row, then per column
//     (goodFeaturesUtils.pyx:49-51).  A parallel scan rounds differently and changes which pixels win,
//     so each row / column chain stays sequential here; parallelism comes from the number of chains
//     (rows x 3 planes, columns x 3 planes), with 64x64 tiles transposed through LDS so that HBM sees
//     coalesced 256-byte segments in both passes.
//   * window sum ((c + a) - b) - d in f32 (:23-31); eigenvalue with the reference's mixed f32/f64
//     arithmetic (:17-19).
//   * candidates are ordered by (val, x, y) descending (selectGoodFeatures.py:234-236): one 64-bit key
//     [f32 bits of val | x:16 | y:16] sorted descending gives exactly that order for val > 0.
//   * _enforceMinimumDistance (selectGoodFeatures.py:45-135) is a sequential greedy pass.  Equivalent
//     form used here: a candidate is accepted iff no previously accepted feature lies within Chebyshev
//     distance mindist-1.  With cells of side mindist at most one accepted feature fits in a cell, so
//     the test reads the 3x3 neighbouring cells of a small grid held in LDS instead of a full-frame map.
// Every shared primitive is defined once, ahead of its first user (key codec, division by a run-time constant and the initial affine
// state in klt_internal.h); a kernel that keeps a copy of its own says so beside the primitive.  Launchers at the end.
#include "klt_internal.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ SAT, the barrier-coupled kernels' pipeline
// What sat_rows_kernel and sat_cols_kernel share: wavefront 0 (`chain`) scans tile t in LDS buffer t & 1 while the loaders put tile t + 1
// into the other buffer (registers -> LDS), fetch tile t + 1 + D into the ring slot that has just become free (global -> registers, a ring
// of D tiles in flight per lane) and store the finished tile t - 1 (LDS -> global).  One barrier per tile.
template <int D, class Fetch, class Put, class Store, class Scan>
__device__ __forceinline__ void sat_tile_pipeline(bool chain, int ntiles, const Fetch &fetch, const Put &put, const Store &store, const Scan &scan)
{
    if (!chain) {
#pragma unroll
        for (int s = 0; s < D; s++) fetch(s, s);
        put(0, 0);
        fetch(0, D);
    }
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += D) {
#pragma unroll
        for (int k = 0; k < D; k++) {
            const int t = t0 + k;
            if (t < ntiles) {                                   // uniform
                if (chain) {
                    scan(k & 1);
                } else {
                    if (t + 1 < ntiles) {
                        put((k + 1) % D, (k + 1) & 1);
                        fetch((k + 1) % D, t + 1 + D);
                    }
                    if (t >= 1) store((k + 1) & 1, t - 1);
                }
                __syncthreads();
            }
        }
    }
    if (!chain) store((ntiles - 1) & 1, ntiles - 1);
}

// ------------------------------------------------------------------ SAT, row pass (+ products)
// The only serial work is the chain itself: 64 dependent f32 adds per 64-column tile and row.  Everything else is kept
// off the chain's wavefront.  block = 5 wavefronts = one band of 16 rows: wavefront 0 runs the 48 chains of the band
// (lane = plane * 16 + row; planes gx*gx, gx*gy, gy*gy) from LDS to LDS; wavefronts 1..4 load gx / gy (coalesced
// 256-byte row segments, a ring of SR_D tiles in flight per lane to cover HBM latency), write the three products of
// the next tile into LDS and store the finished prefix tile of the previous step.  One barrier per tile.
constexpr int SR_ROWS = 16, SR_LD = 68, SR_D = 8, SR_T = 320;

__global__ __launch_bounds__(SR_T) void sat_rows_kernel(const float *__restrict__ gx, const float *__restrict__ gy,
                                                         float *__restrict__ sat, int ncols, int nrows)
{
    __shared__ __attribute__((aligned(16))) float prod[2][3][SR_ROWS * SR_LD];
    __shared__ __attribute__((aligned(16))) float outp[2][3][SR_ROWS * SR_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool chain = tid < 64;
    const int row0 = blockIdx.x * SR_ROWS;
    const int ntiles = (ncols + 63) / 64;
    const size_t plane = (size_t)ncols * nrows;
    const int lr = (tid - 64) >> 6, lc = lane;                 // loader lanes: rows lr, lr + 4, lr + 8, lr + 12 of the band
    float rgx[SR_D][4], rgy[SR_D][4];
    auto fetch = [&](int slot, int t) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int row = row0 + lr + 4 * k, col = t * 64 + lc;
            const bool ok = t < ntiles && row < nrows && col < ncols;
            rgx[slot][k] = ok ? gx[KLT_PIX_STRIDE * ((size_t)row * ncols + col)] : 0.f;      // planes of pixel records (klt_internal.h)
            rgy[slot][k] = ok ? gy[KLT_PIX_STRIDE * ((size_t)row * ncols + col)] : 0.f;
        }
    };
    auto put = [&](int slot, int buf) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int o = (lr + 4 * k) * SR_LD + lc;
            const float a = rgx[slot][k], b = rgy[slot][k];
            prod[buf][0][o] = a * a;
            prod[buf][1][o] = a * b;
            prod[buf][2][o] = b * b;
        }
    };
    auto store = [&](int buf, int t) {
        const int col = t * 64 + lc;
        if (col < ncols) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int r = lr + 4 * k, row = row0 + r;
                if (row < nrows) {
                    sat[(size_t)row * ncols + col] = outp[buf][0][r * SR_LD + lc];
                    sat[plane + (size_t)row * ncols + col] = outp[buf][1][r * SR_LD + lc];
                    sat[2 * plane + (size_t)row * ncols + col] = outp[buf][2][r * SR_LD + lc];
                }
            }
        }
    };
    float carry = 0.f;
    const int cpl = lane >> 4, cr = lane & 15;                 // chain lanes: plane, row (lanes 48..63 idle)
    auto scan = [&](int buf) {
        if (lane < 48) {
            const float4 *a4 = reinterpret_cast<const float4 *>(&prod[buf][cpl][cr * SR_LD]);
            float4 *o4 = reinterpret_cast<float4 *>(&outp[buf][cpl][cr * SR_LD]);
            float4 v[16];
#pragma unroll
            for (int c = 0; c < 16; c++) v[c] = a4[c];
#pragma unroll
            for (int c = 0; c < 16; c++) {
                float4 o;
                carry = carry + v[c].x; o.x = carry;
                carry = carry + v[c].y; o.y = carry;
                carry = carry + v[c].z; o.z = carry;
                carry = carry + v[c].w; o.w = carry;
                o4[c] = o;
            }
        }
    };
    sat_tile_pipeline<SR_D>(chain, ntiles, fetch, put, store, scan);
}

// ------------------------------------------------------------------ SAT, column pass (in place)
// Same structure: block = 32 columns of one plane; wavefront 0 runs the 32 column chains (lane = column) on 32-row
// tiles in LDS, wavefronts 1..4 stream the tiles in (ring of SC_D tiles per lane) and the finished tiles out.
constexpr int SC_COLS = 32, SC_ROWS = 32, SC_D = 12, SC_T = 320;

__global__ __launch_bounds__(SC_T) void sat_cols_kernel(float *__restrict__ sat, int ncols, int nrows)
{
    __shared__ float tin[2][SC_ROWS * SC_COLS], tout[2][SC_ROWS * SC_COLS];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool chain = tid < 64;
    const int x0 = blockIdx.x * SC_COLS;
    float *s = sat + (size_t)blockIdx.y * ncols * nrows;
    const int ntiles = (nrows + SC_ROWS - 1) / SC_ROWS;
    const int lr = (tid - 64) >> 5, lc = (tid - 64) & 31;       // loader lanes: rows lr, lr + 8, lr + 16, lr + 24 of the tile
    float rg[SC_D][4];
    auto fetch = [&](int slot, int t) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int row = t * SC_ROWS + lr + 8 * k, col = x0 + lc;
            rg[slot][k] = (t < ntiles && row < nrows && col < ncols) ? s[(size_t)row * ncols + col] : 0.f;
        }
    };
    auto put = [&](int slot, int buf) {
#pragma unroll
        for (int k = 0; k < 4; k++) tin[buf][(lr + 8 * k) * SC_COLS + lc] = rg[slot][k];
    };
    auto store = [&](int buf, int t) {
        const int col = x0 + lc;
        if (col < ncols) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int r = lr + 8 * k, row = t * SC_ROWS + r;
                if (row < nrows) s[(size_t)row * ncols + col] = tout[buf][r * SC_COLS + lc];
            }
        }
    };
    float carry = 0.f;
    auto scan = [&](int buf) {
        if (lane < SC_COLS) {
            float v[SC_ROWS];
#pragma unroll
            for (int r = 0; r < SC_ROWS; r++) v[r] = tin[buf][r * SC_COLS + lane];
#pragma unroll
            for (int r = 0; r < SC_ROWS; r++) {
                carry = carry + v[r];
                tout[buf][r * SC_COLS + lane] = carry;
            }
        }
    };
    sat_tile_pipeline<SC_D>(chain, ntiles, fetch, put, store, scan);
}

// ------------------------------------------------------------------ seed map for REPLACING_SOME
// selectGoodFeatures.py:64-69: every live feature blocks the square of half-size d around (int(x), int(y))
// The map is stamped, not cleared: a pixel is blocked when it carries THIS selection's stamp (1..255; the host clears the map when the
// stamps wrap or the frame size changes), so that a replacement pass does not begin by zeroing a frame-sized map.
__global__ void seed_fill_kernel(const klt_feat *__restrict__ fl, int nfeat, uint8_t *__restrict__ seedmap,
                                 int ncols, int nrows, int d, uint8_t stamp)
{
    const int f = blockIdx.x;
    if (f >= nfeat) return;
    const klt_feat ft = fl[f];
    if (ft.val < 0) return;
    const int cx = (int)ft.x, cy = (int)ft.y, side = 2 * d + 1;
    for (int k = threadIdx.x; k < side * side; k += blockDim.x) {
        const int ix = cx - d + k % side, iy = cy - d + k / side;
        if (ix >= 0 && ix < ncols && iy >= 0 && iy < nrows) seedmap[(size_t)iy * ncols + ix] = stamp;
    }
}

// A caller's selection mask (klt_set_select_mask*) merged into the seed map: a pixel whose mask byte is 0 gets this selection's stamp, like
// a pixel inside a live feature's square.  Both planes are flat arrays of n = ncols * nrows bytes (a row's end is nothing special; what
// is left is the end of the plane when n % 16 != 0).  Runs on every frame of a masked sequence, so it streams: a lane takes 16 mask bytes
// with one load; a piece without a zero byte writes nothing (and does not read the map), a piece of zero bytes is one 16-byte store of
// stamps, a mixed piece reads the map's 16 bytes and stores the dwords that changed.  The mask is caller memory when it was given as
// a device pointer: its last n % 16 bytes are loaded one by one by a single lane and nothing behind byte n - 1 is read.  The seed map is
// the library's and padded to whole 16-byte pieces (begin_seed_map), so the tail is merged and stored like any other piece.
__device__ __forceinline__ uint32_t zero_bytes(uint32_t w)          // 0xff in every byte of w that is 0
{
    const uint32_t low7 = 0x7f7f7f7fu;
    const uint32_t t = ~(((w & low7) + low7) | w | low7);          // 0x80 in every zero byte
    return (t >> 7) * 0xffu;
}

__device__ __forceinline__ void seed_mask_piece(uint4 m, uint8_t *__restrict__ seed16, uint32_t stamp4)
{
    const uint32_t z[4] = {zero_bytes(m.x), zero_bytes(m.y), zero_bytes(m.z), zero_bytes(m.w)};
    if ((z[0] | z[1] | z[2] | z[3]) == 0u) return;
    uint4 *const out = reinterpret_cast<uint4 *>(seed16);
    if ((z[0] & z[1] & z[2] & z[3]) == 0xffffffffu) { *out = make_uint4(stamp4, stamp4, stamp4, stamp4); return; }
    const uint4 s = *out;
    const uint32_t old[4] = {s.x, s.y, s.z, s.w};
    uint32_t *const w = reinterpret_cast<uint32_t *>(seed16);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (z[k]) w[k] = (old[k] & ~z[k]) | (stamp4 & z[k]);
}

__global__ __launch_bounds__(256) void seed_mask_kernel(const uint8_t *__restrict__ mask, uint8_t *__restrict__ seedmap, size_t n, uint8_t stamp)
{
    const uint32_t stamp4 = 0x01010101u * stamp;
    const size_t pieces = n / 16;
    const uint4 *const m16 = reinterpret_cast<const uint4 *>(mask);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (size_t)gridDim.x * 256)
        seed_mask_piece(m16[i], seedmap + 16 * i, stamp4);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255 && (n & 15)) {      // the plane's last n % 16 bytes: bytes behind the end count as "allowed"
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w[k] = ~0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const size_t b = 16 * pieces + 4 * k + j;
                if (b < n && mask[b] == 0) w[k] &= ~(0xffu << (8 * j));
            }
        }
        seed_mask_piece(make_uint4(w[0], w[1], w[2], w[3]), seedmap + 16 * pieces, stamp4);
    }
}

// ------------------------------------------------------------------ eigenvalue map + sort keys
__device__ __forceinline__ float window_sum(const float *__restrict__ s, int ncols, int x, int y, int hw, int hh)
{
    const float a = s[(size_t)(y - hh - 1) * ncols + (x - hw - 1)];
    const float b = s[(size_t)(y - hh - 1) * ncols + (x + hw)];
    const float c = s[(size_t)(y + hh) * ncols + (x + hw)];
    const float d = s[(size_t)(y + hh) * ncols + (x - hw - 1)];
    return ((c + a) - b) - d;
}

// Candidate cell (xi, yi) of the lattice -> its pixel (SelectArgs and MisArgs name the lattice alike), and "this pixel cannot be placed":
// it carries this selection's stamp in the seed map (a live feature's square, or a selection mask's zero).
// (mask_hist_kernel keeps its own copy of both: through these it takes 33 SGPRs instead of 32.)
template <class Args> __device__ __forceinline__ int cell_x(const Args &a, int xi) { return a.bx + xi * a.step; }
template <class Args> __device__ __forceinline__ int cell_y(const Args &a, int yi) { return a.by + yi * a.step; }
template <class Args> __device__ __forceinline__ size_t cell_pixel(const Args &a, int xi, int yi) { return (size_t)cell_y(a, yi) * a.ncols + cell_x(a, xi); }
__device__ __forceinline__ bool seed_blocked(const uint8_t *__restrict__ seed, uint8_t stamp, size_t pixel) { return seed[pixel] == stamp; }

// key of candidate k (0 = not a candidate); also stores the eigenvalue
__device__ __forceinline__ unsigned long long eigen_key(const SelectArgs &a, int k)
{
    const int xi = k % a.nx, yi = k / a.nx;
    const int x = cell_x(a, xi), y = cell_y(a, yi);
    // REPLACING_SOME: a pixel inside the exclusion square of a live feature can never be placed (selectGoodFeatures.py:64-69 marks
    // the feature map before the walk), so it is not scored at all -- most of the frame when few features were lost
    if (a.seedmap && seed_blocked(a.seedmap, a.seed_stamp, cell_pixel(a, xi, yi))) { if (a.valmap) a.valmap[k] = 0.f; return 0ull; }
    const size_t plane = (size_t)a.ncols * a.nrows;
    const float gxx = window_sum(a.sat, a.ncols, x, y, a.hw, a.hh);
    const float gxy = window_sum(a.sat + plane, a.ncols, x, y, a.hw, a.hh);
    const float gyy = window_sum(a.sat + 2 * plane, a.ncols, x, y, a.hw, a.hh);
    float val;
    unsigned long long key = klt_window_key(gxx, gxy, gyy, a.min_eig, x, y, &val);       // goodFeaturesUtils.pyx:17-19 (klt_internal.h)
    if (a.val_in) {                                                                      // test hook: the eigenvalue is given
        val = a.val_in[k];
        key = (double)val >= a.min_eig ? klt_pack_key(val, x, y) : 0ull;
    }
    if (a.valmap) a.valmap[k] = val;
    return key;
}

__global__ __launch_bounds__(256) void eigen_kernel(SelectArgs a)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.npow2) return;
    a.keys[k] = k < a.nx * a.ny ? eigen_key(a, k) : 0ull;     // padding sorts last
}

// ------------------------------------------------------------------ top-K prefilter for the sort
// The greedy pass only ever looks at a prefix of the sorted candidates (197 775 of 1 411 200 at 1080p for 5000
// features).  A 8192-bin histogram over the top 13 bits of the (positive) f32 eigenvalue picks the smallest bin
// boundary that keeps at least `target` candidates; only those are compacted and sorted.  Order inside the kept set
// is unchanged (same keys), so the walk sees exactly the same prefix; if it ever runs off the end of the kept set
// before the list is full, the host repeats the selection with the full sort.
constexpr int HIST_BINS = 8192;
__device__ __forceinline__ unsigned key_bin(unsigned long long key) { return (klt_key_bits(key) >> 18) & (HIST_BINS - 1); }

// a workgroup's (256 threads) histogram in LDS: cleared, counted by the kernel's own loop (LDS atomics), its non-empty bins added to the global one
__device__ __forceinline__ void hist_clear(unsigned *h)
{
    for (int i = threadIdx.x; i < HIST_BINS; i += 256) h[i] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void hist_flush(const unsigned *h, unsigned *__restrict__ hist)
{
    __syncthreads();
    for (int i = threadIdx.x; i < HIST_BINS; i += 256)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// stride > 1: every stride-th key only (an estimate is enough where the threshold is just a work-saving cut)
__global__ __launch_bounds__(256) void key_hist_kernel(const unsigned long long *__restrict__ keys, int n, unsigned *__restrict__ hist, int stride)
{
    __shared__ unsigned h[HIST_BINS];
    hist_clear(h);
    for (int i = (blockIdx.x * 256 + threadIdx.x) * stride; i < n; i += gridDim.x * 256 * stride) {
        const unsigned long long key = keys[i];
        if (key) atomicAdd(&h[key_bin(key)], 1u);
    }
    hist_flush(h, hist);
}

// info[0] = threshold bin, info[1] = number of keys in bins >= threshold, info[2] = number of valid keys
// slots != nullptr: target = max(target, per_slot * *slots) -- REPLACING_SOME sizes the cut by the number of lost features, which
// only the device knows (mis_prepare_kernel)
__global__ __launch_bounds__(1024) void key_threshold_kernel(const unsigned *__restrict__ hist, unsigned target, unsigned *__restrict__ info,
                                                             const int *__restrict__ slots, unsigned per_slot)
{
    __shared__ unsigned suf[1025];
    const int t = threadIdx.x;
    if (slots) {
        const unsigned want = per_slot * (unsigned)max(*slots, 0);
        target = want > target ? want : target;
    }
    unsigned mine = 0;
    for (int b = 0; b < 8; b++) mine += hist[8 * t + b];
    suf[t] = mine;
    if (t == 0) suf[1024] = 0u;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {             // inclusive suffix scan: suf[t] = sum of parts t..1023
        const unsigned v = t + off < 1024 ? suf[t + off] : 0u;
        __syncthreads();
        suf[t] += v;
        __syncthreads();
    }
    const unsigned total = suf[0];
    if (total < target) {
        if (t == 0) { info[0] = 0u; info[1] = total; info[2] = total; }
        return;
    }
    if (suf[t] >= target && suf[t + 1] < target) {         // the boundary lies inside this thread's 8 bins
        unsigned acc = suf[t + 1];
        int b = 8 * t + 7;
        for (; b > 8 * t; b--) {
            acc += hist[b];
            if (acc >= target) break;
        }
        if (b == 8 * t) acc = suf[t];
        info[0] = (unsigned)b; info[1] = acc; info[2] = total;
    }
}

// Eigenvalues, keys, and -- for the parallel minimum-distance passes -- the histogram behind the prefilter threshold in the
// same launch: every 4th workgroup histograms its keys (an estimate is enough: the threshold only saves work, any value
// is correct -- as long as the repeat does not rest on the sample's counts: mis_init_kernel reports what the bin really
// dropped); key_threshold_kernel turns it into the threshold bin.  a.hist == nullptr: keys only.
__global__ __launch_bounds__(256) void eigen_hist_kernel(SelectArgs a)
{
    __shared__ unsigned h[HIST_BINS];
    const int tid = threadIdx.x, ncand = a.nx * a.ny;
    // (XCD-contiguous eighths of the candidates instead of this interleaved sweep -- the table rows shared by windows 2 hh + 1 rows
    // apart then meet in one L2 -- were measured in round 2: no change, 14.6 us at 1080p either way)
    const bool sampler = a.hist != nullptr && (blockIdx.x & 3) == 0;
    if (sampler) hist_clear(h);
    for (int k = blockIdx.x * 256 + tid; k < ncand; k += gridDim.x * 256) {
        const unsigned long long key = eigen_key(a, k);
        a.keys[k] = key;
        if (sampler && key) atomicAdd(&h[key_bin(key)], 1u);
    }
    if (!a.hist) return;
    if (sampler) hist_flush(h, a.hist);
}

// Keys scored ahead of time without the seed map (klt_select_prepare_async): the histogram behind the cut counts the keys outside
// the live features' squares, on a sample of every 16th block of 256 keys (the cut only saves work; its targets are scaled to the
// sample).  A workgroup takes eight sampled blocks in one step: the seed-map loads, then the key loads of the cells outside the squares,
// are in flight together, and only ~250 workgroups flush their bins (one block per step and every 4th block, as eigen_hist_kernel
// samples, read 29-35 us for a 4K frame: two dependent round trips per block, then 1024 workgroups adding to the same few hundred words).
constexpr int MASK_HIST_SAMPLE = 16;
__global__ __launch_bounds__(256) void mask_hist_kernel(SelectArgs a)
{
    __shared__ unsigned h[HIST_BINS];
    const int tid = threadIdx.x, ncand = a.nx * a.ny;
    hist_clear(h);
    constexpr int U = 8, S = MASK_HIST_SAMPLE;
    for (int k0 = S * U * blockIdx.x * 256 + tid; k0 < ncand; k0 += S * U * gridDim.x * 256) {
        unsigned long long key[U];
        uint8_t masked[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int k = k0 + S * u * 256, xi = k % a.nx, yi = k / a.nx;
            masked[u] = k < ncand ? (uint8_t)(a.seedmap[(size_t)(a.by + yi * a.step) * a.ncols + a.bx + xi * a.step] == a.seed_stamp) : (uint8_t)1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            key[u] = masked[u] ? 0ull : a.keys[k0 + S * u * 256];
            if (!key[u]) masked[u] = 1;
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (!masked[u]) atomicAdd(&h[key_bin(key[u])], 1u);
    }
    hist_flush(h, a.hist);
}

// Wavefront-ordered compaction: the lanes that keep their element get consecutive slots, in lane order, behind a range that lane 0
// reserves on an LDS cursor.  Every lane calls.  (nms_kernel needs rank order ACROSS wavefronts and counts per wavefront: another algorithm.)
__device__ __forceinline__ unsigned wave_compact_slot(bool keep, unsigned *cursor, int lane)
{
    const unsigned long long m = __ballot(keep);
    unsigned wbase = 0;
    if (lane == 0 && m) wbase = atomicAdd(cursor, (unsigned)__popcll(m));
    wbase = __shfl(wbase, 0);
    return wbase + __popcll(m & ((1ull << lane) - 1ull));
}

// Order inside the kept set does not matter (it is sorted next), so every workgroup counts the keys it keeps in its
// contiguous chunk, reserves a range with ONE global atomic (a returning atomic on a single word sustains only ~90 per
// microsecond chip-wide), and fills the range using an LDS cursor.
__global__ __launch_bounds__(256) void key_compact_kernel(const unsigned long long *__restrict__ keys, int n,
                                                           const unsigned *__restrict__ info, unsigned long long *__restrict__ out,
                                                           unsigned *__restrict__ counter)
{
    __shared__ unsigned s_count, s_base, s_cursor;
    const unsigned thr = info[0];
    const int lane = threadIdx.x & 63;
    const int chunk = ((n + gridDim.x - 1) / gridDim.x + 255) & ~255;
    const int begin = blockIdx.x * chunk, end = min(n, begin + chunk);
    if (threadIdx.x == 0) { s_count = 0u; s_cursor = 0u; }
    __syncthreads();
    unsigned mine = 0;
    for (int i = begin + threadIdx.x; i < end; i += 256) {
        const unsigned long long key = keys[i];
        mine += (key != 0ull && key_bin(key) >= thr) ? 1u : 0u;
    }
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if (lane == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_count ? atomicAdd(counter, s_count) : 0u;
    __syncthreads();
    if (s_count == 0u) return;
    const unsigned base = s_base;
    for (int i0 = begin; i0 < end; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const unsigned long long key = i < end ? keys[i] : 0ull;
        const bool keep = key != 0ull && key_bin(key) >= thr;
        const unsigned slot = wave_compact_slot(keep, &s_cursor, lane);
        if (keep) out[base + slot] = key;
    }
}

// ------------------------------------------------------------------ bitonic sort, descending, u64 keys
constexpr int SORT_E = 2048;      // keys per workgroup (16 KiB of LDS)
constexpr int SORT_T = 1024;

// compare-exchange; true when the two were swapped
__device__ __forceinline__ bool cmpx(unsigned long long &a, unsigned long long &b, bool desc)
{
    const bool sw = desc ? (a < b) : (a > b);
    if (sw) { const unsigned long long t = a; a = b; b = t; }
    return sw;
}

// a workgroup's 2048-key chunk in LDS: in, one compare-exchange step with partner distance j of the stage that builds runs of length k, out
__device__ __forceinline__ void bitonic_lds_load(unsigned long long *s, const unsigned long long *keys, size_t base, int t)
{
    s[t] = keys[base + t]; s[t + SORT_T] = keys[base + t + SORT_T];
    __syncthreads();
}
__device__ __forceinline__ void bitonic_lds_step(unsigned long long *s, size_t base, int t, int j, int k)
{
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    const int l = i | j;
    const bool desc = (((base + i) & (size_t)k) == 0);
    unsigned long long a = s[i], b = s[l];
    cmpx(a, b, desc);
    s[i] = a;
    s[l] = b;
    __syncthreads();
}
__device__ __forceinline__ void bitonic_lds_store(const unsigned long long *s, unsigned long long *keys, size_t base, int t)
{
    keys[base + t] = s[t]; keys[base + t + SORT_T] = s[t + SORT_T];
}

// full sort of each 2048-key chunk; chunk direction follows the global network (bit 11 of the index)
__global__ __launch_bounds__(SORT_T) void bitonic_local_sort(unsigned long long *__restrict__ keys)
{
    __shared__ unsigned long long s[SORT_E];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SORT_E;
    bitonic_lds_load(s, keys, base, t);
    for (int k = 2; k <= SORT_E; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) bitonic_lds_step(s, base, t, j, k);
    bitonic_lds_store(s, keys, base, t);
}

// one compare-exchange step with partner distance j >= SORT_E, inside the stage that builds runs of length k
__global__ __launch_bounds__(256) void bitonic_global_step(unsigned long long *__restrict__ keys, int j, int k, int half_n)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= half_n) return;
    const size_t i = ((size_t)(t & ~(j - 1)) << 1) | (size_t)(t & (j - 1));
    const size_t l = i | (size_t)j;
    const bool desc = ((i & (size_t)k) == 0);
    unsigned long long a = keys[i], b = keys[l];
    if (cmpx(a, b, desc)) { keys[i] = a; keys[l] = b; }
}

// the remaining steps (j = 1024 .. 1) of stage k, inside LDS
__global__ __launch_bounds__(SORT_T) void bitonic_local_merge(unsigned long long *__restrict__ keys, int k)
{
    __shared__ unsigned long long s[SORT_E];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * SORT_E;
    bitonic_lds_load(s, keys, base, t);
    for (int j = SORT_E >> 1; j > 0; j >>= 1) bitonic_lds_step(s, base, t, j, k);
    bitonic_lds_store(s, keys, base, t);
}

// ------------------------------------------------------------------ greedy minimum-distance pass
// One workgroup of 16 wavefronts walks the sorted keys 1024 at a time:
//   1. every thread tests its candidate against the cell grid as it stood at the start of the super-batch
//      (almost every candidate dies here: it is blocked by a feature accepted long before);
//   2. the survivors are compacted in rank order;
//   3. wave 0 resolves them sequentially with ballots -- a survivor can only be blocked by a feature accepted
//      inside the same super-batch, which is a register compare (plus a grid re-test for survivors beyond the
//      first 64, whose predecessors in the super-batch are already in the grid).
// The result is exactly the sequential walk of selectGoodFeatures.py:71-134.
constexpr int NMS_T = 1024;

template <bool LDSGRID>
__device__ __forceinline__ uint32_t grid_load(const uint32_t *p)
{
    if (LDSGRID) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // L2-served: never a stale L1 line
}

// x / cell (klt_div_magic, klt_internal.h; coordinates are below 65536)
__device__ __forceinline__ int cell_of(int v, const NmsArgs &a)
{
    return a.cell == 1 ? v : (int)klt_div_by_magic((unsigned)v, a.cell_magic);
}

template <bool LDSGRID>
__device__ __forceinline__ bool grid_free(const uint32_t *grid, const NmsArgs &a, int x, int y)
{
    const int cx = cell_of(x, a), cy = cell_of(y, a);
    bool ok = true;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int gx = cx + dx, gy = cy + dy;
            if (gx < 0 || gy < 0 || gx >= a.gw || gy >= a.gh) continue;
            const uint32_t v = grid_load<LDSGRID>(&grid[gy * a.gw + gx]);
            if (v) {
                const int ax = (int)((v - 1u) >> 16), ay = (int)((v - 1u) & 0xffffu);
                if (abs(x - ax) <= a.d && abs(y - ay) <= a.d) ok = false;
            }
        }
    return ok;
}

// slot `slot` of the list filled from an accepted candidate's key; the slot's affine state starts over when the list has one
__device__ __forceinline__ void fill_slot(const NmsArgs &a, int slot, unsigned long long key)
{
    klt_feat ft;
    ft.x = (float)klt_key_x(key);
    ft.y = (float)klt_key_y(key);
    ft.val = (int32_t)klt_key_val(key);                                      // int(val), selectGoodFeatures.py:119
    ft.aux = 0;
    a.fl[slot] = ft;
    if (a.aff_rec) a.aff_rec[slot] = klt_affine_rec_initial();
}

// a slot the candidates did not reach: selectGoodFeatures.py:78-94 (SELECTING_ALL only; DESIGN.md lists the deviation)
__device__ __forceinline__ void mark_not_found(klt_feat *fl, int slot)
{
    klt_feat ft;
    ft.x = -1.f; ft.y = -1.f; ft.val = KLT_NOT_FOUND; ft.aux = 0;
    fl[slot] = ft;
}

// The walk under a per-cell quota (klt_set_select_grid, QUOTA): a candidate accepted by distance marks the cell grid and blocks the later
// lanes near it whatever its cell holds; it takes a slot, and room, only while its cell has room left.  The room of a batch of 64
// survivors: what the cell had when the batch began (g.live, which the batch's placed features are added to behind it) minus the lanes
// of the same cell placed before this one.  The kernel argument is one struct per QUOTA value: the plain walk receives NmsArgs alone.
struct NmsQuotaArgs : NmsArgs { QuotaArgs g; };
template <bool QUOTA>
using NmsKernArgs = std::conditional_t<QUOTA, NmsQuotaArgs, NmsArgs>;

__device__ __forceinline__ int quota_cell(const QuotaArgs &g, int x, int y)
{
    const int cx = g.cw == 1 ? x : (int)klt_div_by_magic((unsigned)x, g.cw_magic);
    const int cy = g.ch == 1 ? y : (int)klt_div_by_magic((unsigned)y, g.ch_magic);
    return cy * g.gw + cx;
}

// room left in a cell; the count is read from L2 (the walk adds to it between two reads)
__device__ __forceinline__ int quota_left(const QuotaArgs &g, int cell)
{
    const unsigned held = __hip_atomic_load(&g.live[cell], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return held < (unsigned)g.q ? (int)((unsigned)g.q - held) : 0;
}

// The slots that may be filled when the list is not overwritten, in list order (selectGoodFeatures.py:109-110): the slots whose feature
// is lost.  a.slots[k] = index of the k-th fillable slot; returns how many there are.  Every thread of the workgroup calls.
__device__ __forceinline__ int list_free_slots(const NmsArgs &a, int *scan, int *s_nfill, int tid)
{
    const int per = (a.nfeat + NMS_T - 1) / NMS_T, lo = tid * per, hi = min(lo + per, a.nfeat);
    int cnt = 0;
    for (int i = lo; i < hi; i++) cnt += a.fl[i].val < 0;
    scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < NMS_T; off <<= 1) {          // Hillis-Steele inclusive scan
        const int v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int k = scan[tid] - cnt;
    for (int i = lo; i < hi; i++)
        if (a.fl[i].val < 0) a.slots[k++] = i;
    if (tid == NMS_T - 1) *s_nfill = scan[tid];
    __syncthreads();
    return *s_nfill;
}

// Steps 1 and 2 on one super-batch: the candidates that pass the first test go to surv[] in rank order; returns how many.
// ended: some thread held a zero key -- everything after it is padding.  Every thread of the workgroup calls.
template <bool LDSGRID, bool QUOTA>
__device__ __forceinline__ int first_test_compact(const NmsKernArgs<QUOTA> &a, const uint32_t *grid, unsigned long long cur,
                                                  unsigned long long *surv, int *wave_cnt, int lane, int wave, int &ended)
{
    const bool valid = cur != 0ull;
    const int x = klt_key_x(cur), y = klt_key_y(cur);
    bool ok = valid;
    if constexpr (QUOTA) {
        if (valid) ok = a.d >= 0 ? grid_free<LDSGRID>(grid, a, x, y) : quota_left(a.g, quota_cell(a.g, x, y)) > 0;
    } else {
        if (valid && a.d >= 0) ok = grid_free<LDSGRID>(grid, a, x, y);
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    ended = __syncthreads_or(!valid);
    int offset = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NMS_T / 64; w++) {
        const int c = wave_cnt[w];
        offset += w < wave ? c : 0;
        total += c;
    }
    if (ok) surv[offset + __popcll(m & ((1ull << lane) - 1ull))] = cur;
    __syncthreads();
    return total;
}

// an accepted candidate in the cell grid: it blocks what comes after it within the exclusion square
template <bool LDSGRID>
__device__ __forceinline__ void grid_mark(uint32_t *grid, const NmsArgs &a, int x, int y)
{
    const uint32_t code = (((uint32_t)x << 16) | (uint32_t)y) + 1u;
    uint32_t *cellp = &grid[cell_of(y, a) * a.gw + cell_of(x, a)];
    if (LDSGRID) *cellp = code;
    else __hip_atomic_store(cellp, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Step 3 on one batch of 64 survivors, one per lane of wave 0 (k = 0: none): `placed` slots are taken and at most nfill may be;
// returns how many this batch takes.  retest: earlier batches of the super-batch are in the grid and were not there for the first test.
template <bool LDSGRID, bool QUOTA>
__device__ __forceinline__ int resolve_batch(const NmsKernArgs<QUOTA> &a, uint32_t *grid, unsigned long long k, bool retest, int placed,
                                             int nfill, int lane)
{
    const int sx = klt_key_x(k), sy = klt_key_y(k);
    bool is_free = k != 0ull;
    if (retest && is_free && a.d >= 0) is_free = grid_free<LDSGRID>(grid, a, sx, sy);
    int qc = -1, left = 0;                           // QUOTA: the lane's cell and the room it had when the batch began
    if constexpr (QUOTA) {
        if (is_free) { qc = quota_cell(a.g, sx, sy); left = quota_left(a.g, qc); }
    }
    unsigned long long mask = __ballot(is_free), accepted = 0ull, taken = 0ull;       // accepted by distance; of those, the ones that take a slot
    int room = nfill - placed;
    if constexpr (!QUOTA) {
        if (a.d < 0) {                   // nothing excludes anything: the first `room` free lanes are accepted
            const bool take = ((mask >> lane) & 1ull) && __popcll(mask & ((1ull << lane) - 1ull)) < room;
            accepted = __ballot(take);
            mask = 0ull;
        }
    }
    // rank order = lane order: the first free lane is accepted and blocks the later lanes near it
    while (mask != 0ull && room > 0) {
        const int l = __ffsll((long long)mask) - 1;
        accepted |= 1ull << l;
        if constexpr (!QUOTA) room--;
        mask &= ~(1ull << l);
        if constexpr (QUOTA) {
            const int cell_l = __builtin_amdgcn_readlane(qc, l), left_l = __builtin_amdgcn_readlane(left, l);
            const unsigned long long same = __ballot(qc == cell_l);
            if (__popcll(taken & same) < left_l) { taken |= 1ull << l; room--; }
        }
        if (a.d >= 0) {
            const int ax = __builtin_amdgcn_readlane(sx, l), ay = __builtin_amdgcn_readlane(sy, l);
            mask &= ~__ballot(abs(sx - ax) <= a.d && abs(sy - ay) <= a.d);
        }
    }
    if constexpr (!QUOTA) {
        taken = accepted;
        if ((accepted >> lane) & 1ull) {
            const int rank = placed + __popcll(accepted & ((1ull << lane) - 1ull));
            fill_slot(a, a.overwrite_all ? rank : a.slots[rank], k);
            if (a.d >= 0) grid_mark<LDSGRID>(grid, a, sx, sy);
        }
    } else {
        if (((accepted >> lane) & 1ull) && a.d >= 0) grid_mark<LDSGRID>(grid, a, sx, sy);
        if ((taken >> lane) & 1ull) {
            const int rank = placed + __popcll(taken & ((1ull << lane) - 1ull));
            fill_slot(a, a.overwrite_all ? rank : a.slots[rank], k);
            __hip_atomic_fetch_add(&a.g.live[qc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return __popcll(taken);
}

// the end of the walk (wave 0): the slots the candidates did not reach, and the outcome
__device__ __forceinline__ void walk_tail(const NmsArgs &a, int placed, bool list_full, int lane)
{
    if (!list_full && a.overwrite_all)                         // candidates exhausted
        for (int i = placed + lane; i < a.nfeat; i += 64) mark_not_found(a.fl, i);
    if (lane == 0 && a.placed_out) {
        a.placed_out[0] = placed;
        a.placed_out[1] = list_full ? 0 : 1;      // 1: the walk ran out of candidates before the list was full
    }
}

template <bool LDSGRID, bool QUOTA>
__global__ __launch_bounds__(NMS_T) void nms_kernel(NmsKernArgs<QUOTA> a)
{
    extern __shared__ uint32_t lds_grid[];
    __shared__ unsigned long long surv[NMS_T];
    __shared__ int wave_cnt[NMS_T / 64];
    __shared__ int scan[NMS_T];
    __shared__ int s_stop, s_nfill;
    uint32_t *grid = LDSGRID ? lds_grid : a.grid_global;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDSGRID)
        for (int i = tid; i < a.gw * a.gh; i += NMS_T) grid[i] = 0u;
    if (tid == 0) s_stop = 0;
    const int nfill = a.overwrite_all ? a.nfeat : list_free_slots(a, scan, &s_nfill, tid);      // overwriting: every slot, in order
    __syncthreads();

    int placed = 0;                               // meaningful in wave 0 only
    bool list_full = nfill == 0;
    unsigned long long key = tid < a.nkeys ? a.keys[tid] : 0ull;
    for (int pos = 0; pos < a.nkeys && nfill > 0; pos += NMS_T) {
        const unsigned long long cur = key;
        const int nxt = pos + NMS_T + tid;
        key = nxt < a.nkeys ? a.keys[nxt] : 0ull;                 // prefetch the next super-batch
        int ended;
        const int total = first_test_compact<LDSGRID, QUOTA>(a, grid, cur, surv, wave_cnt, lane, wave, ended);
        if (wave == 0) {
            for (int base = 0; base < total && !list_full; base += 64) {
                const unsigned long long k = base + lane < total ? surv[base + lane] : 0ull;
                placed += resolve_batch<LDSGRID, QUOTA>(a, grid, k, base > 0, placed, nfill, lane);
                if (placed >= nfill) list_full = true;                            // :112
                // the next batch, and the next first test, read the grid -- and under a quota g.live, which lives in global memory
                if constexpr (QUOTA) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            }
            if (lane == 0 && (list_full || ended)) s_stop = 1;
        }
        __syncthreads();
        if (s_stop) break;
    }
    if (wave == 0) walk_tail(a, placed, list_full, lane);
}

// ------------------------------------------------------------------ minimum distance without the serial walk
// _enforceMinimumDistance (selectGoodFeatures.py:45-135) accepts a candidate iff no candidate of higher rank within
// the exclusion square was accepted.  That fixed point is unique, so it can be reached in any order: a candidate is
// ACCEPTED as soon as every higher-ranked candidate within the square is rejected, and REJECTED as soon as one
// accepted candidate lies within the square.  Every decision taken is final and equals the sequential walk's; stale
// reads of a neighbour (still "undecided" although it has just been decided) only postpone a decision.  One launch =
// one such pass over the undecided candidates; 6 passes settle 320 000 candidates of a 1080p frame.  The accepted
// candidates are then sorted by rank and the first `free slots` of them are exactly what the walk would have placed.
//
// State per candidate cell (u32): 0 = no candidate / rejected, f32 bits of the eigenvalue (>= 1.0f) = undecided,
// bits | 0x80000000 = accepted.  Rank order = (value, x, y) descending, so for equal values the neighbour to the right
// wins, and in the same column the neighbour below.
// Each workgroup owns one 32x32 tile of the candidate grid and the list of its undecided cells (compacted in place).
constexpr int MIS_TILE = 32, MIS_CAP = MIS_TILE * MIS_TILE, MIS_T = 256;

// Workgroup -> tile.  Workgroup b runs on XCD b % 8: XCD k takes the k-th contiguous eighth of the (row-major) tiles, so that the
// halo cells a tile shares with its neighbours come out of the same L2.
__device__ __forceinline__ void xcd_range(unsigned k, unsigned g, unsigned &first, unsigned &len)     // XCD k's eighth of g tiles
{
    const unsigned base = g >> 3, rem = g & 7u;
    first = k * base + min(k, rem); len = base + (k < rem ? 1u : 0u);
}
__device__ __forceinline__ unsigned xcd_tile(unsigned b, unsigned g)          // the tile of workgroup b of g, one tile per workgroup
{
    unsigned first, len;
    xcd_range(b & 7u, g, first, len);
    return first + (b >> 3);
}

__global__ __launch_bounds__(MIS_T) void mis_init_kernel(MisArgs a)
{
    __shared__ unsigned s_cursor;
    const int tiles_x = (a.nx + MIS_TILE - 1) / MIS_TILE;
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const unsigned thr = a.info[0];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) s_cursor = 0u;
    __syncthreads();
    uint32_t *list = a.list + (size_t)tile * MIS_CAP;
    // the four cells of a thread: seed-map bytes first (keys scored ahead of time carry no mask), then the keys of the cells outside
    // the live features' squares, each group of loads in flight together
    constexpr int U = MIS_CAP / MIS_T;
    bool inside[U];
    int pcell[U];
    unsigned long long key[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int k = u * MIS_T + threadIdx.x;
        const int xi = tx * MIS_TILE + (k & (MIS_TILE - 1)), yi = ty * MIS_TILE + k / MIS_TILE;
        inside[u] = xi < a.nx && yi < a.ny;
        pcell[u] = yi * a.nx + xi;
        key[u] = 1ull;
        if (inside[u] && a.seed) key[u] = seed_blocked(a.seed, a.seed_stamp, cell_pixel(a, xi, yi)) ? 0ull : 1ull;
    }
#pragma unroll
    for (int u = 0; u < U; u++) key[u] = inside[u] && key[u] ? a.keys[pcell[u]] : 0ull;
    bool dropped = false;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int p = pcell[u];
        const bool keep = key[u] != 0ull && key_bin(key[u]) >= thr;
        dropped |= key[u] != 0ull && !keep;
        if (inside[u]) a.st[p] = keep ? klt_key_bits(key[u]) : 0u;
        const unsigned slot = wave_compact_slot(keep, &s_cursor, lane);
        if (keep) list[slot] = (uint32_t)p;
    }
    // the cut kept a valid key of this tile out of the passes: what the repeat with every candidate rests on (the histogram behind the cut
    // is a sample, and its counts say nothing about the keys it did not see).  A plain store of 1, like "something is left" in a pass.
    if (__ballot(dropped) != 0ull && lane == 0) *a.cut_dropped = 1u;
    __syncthreads();
    if (threadIdx.x == 0) a.cnt[tile] = s_cursor;
}

// (Several passes per launch -- every tile looping over re-staged states read with agent-scope loads, so that decisions of
// other XCDs are seen inside the launch -- were measured in round 2: 2 launches x 41 us instead of 6 x 13 us at 1080p, i.e. the
// same; at 4K, where the 5700 tiles are not all resident, the early tiles spin on neighbours that have not started: 218 vs 99 us.
// A pass costs what it computes (staging + window maxima of every active tile, ~4.6 M wavefront-instructions), not its launch.)
// Timeline of one workgroup in the first pass (1080p cfg-2 frame, 1431 tiles, ~220 candidates each; medians, wall clock read by
// thread 0 at the stage boundaries): list length 0.4 us, staging the tile 4.1, window maxima 1.3, decisions 2.2, tie checks 1.7, push
// 1.0, keys 0.3 -- 11 us, and 16.8 us from the first workgroup's start to the last one's end; in the fifth pass (145 tiles, ~3
// candidates) 0.4 / 2.0 / 0.8 / 0.9 / 0.2 / 0.1 / 0.1 -- 4.4 us in a 7.4 us launch.  Staging is state-map reads that missed the L2
// (every kernel boundary invalidates it): hence the XCD-contiguous tile order below (-4 % on a 4K frame).
// RC > 0: the exclusion radius as a compile-time constant (the reference's default mindist 10 -> 9 cells: tile geometry, window
// loops and the index arithmetic fold); RC = 0: any radius
template <int RC>
__device__ __forceinline__ void mis_round_tile(const MisArgs &a, int round, unsigned tile, unsigned n)
{
    // staged tiles: S = states of the tile + halo ((32 + 2R)^2 u32), H = per row of S and interior column the maximum
    // state over the horizontal window; a candidate then needs the 2R + 1 values of H above and below it.  The maximum
    // carries the accepted bit.  States compare like the rank except for equal eigenvalues: a candidate whose value
    // equals the window maximum scans the window for an equal neighbour of higher rank (right of it, or below it in
    // the same column).
    extern __shared__ uint32_t lds32[];
    __shared__ unsigned short top_local[MIS_CAP], wait_local[MIS_CAP];
    __shared__ unsigned s_cursor, s_acc, s_top, s_left;
    const unsigned have = a.acc_cnt[tile];             // accepted candidates of this tile so far
    const int tiles_x = (a.nx + MIS_TILE - 1) / MIS_TILE;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int R = RC > 0 ? RC : a.R, W = MIS_TILE + 2 * R, L = 2 * R + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (Deciding the last few candidates of a tile without staging it -- a wavefront reading each candidate's window straight from
    // the states -- was measured in round 2: every pass got slower, 11.3 vs 7.4 us for the late ones; the dependent L2 round trips
    // per candidate cost more than staging the tile once.)
    const bool staged = a.stage && R > 0;
    uint32_t *H = lds32;                      // [W][32]
    uint32_t *S = lds32 + W * MIS_TILE;       // [W][W]
    // candidates accepted in this pass: at most a.acc_cap per tile (pairwise more than R cells apart), behind the staged tiles
    // (eight workgroups per CU instead of seven -- 2048 slots for the tiles of a 1080p frame -- were measured this way: no change)
    unsigned short *acc_local = reinterpret_cast<unsigned short *>(lds32 + (staged ? W * MIS_TILE + W * W : 0));
    const int ox = tx * MIS_TILE - R, oy = ty * MIS_TILE - R;
    // a cell of the tile travels through LDS as q = ly * 32 + lx (tile-local coordinates); its index in the lattice
    struct Local { int lx, ly; };
    auto local_of = [](int q) { return Local{q % MIS_TILE, q / MIS_TILE}; };
    auto cell_of_local = [&](int lx, int ly) { return (ty * MIS_TILE + ly) * a.nx + tx * MIS_TILE + lx; };
    uint32_t *list = a.list + (size_t)tile * MIS_CAP;
    unsigned next_p = threadIdx.x < n ? list[threadIdx.x] : 0u;           // first batch, in flight during the staging
    if (threadIdx.x == 0) { s_acc = 0u; s_cursor = 0u; s_top = 0u; s_left = 0u; }
    // tile + halo inside the frame (all but the tiles along its edges): no test per cell -- column test once per lane, row test on the
    // wavefront's (scalar) number; the general loop below spends a dozen instructions per load on them
    const bool interior = staged && ox >= 0 && oy >= 0 && ox + W <= a.nx && oy + W <= a.ny;
    if (interior) {
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        for (int cx0 = 0; cx0 < W; cx0 += 64) {
            const int cx = cx0 + lane;
            if (cx < W) {
                const uint32_t *col = a.st + ((unsigned)oy * (unsigned)a.nx + (unsigned)(ox + cx));
                for (int r0 = 0; r0 < W; r0 += 64) {
                    uint32_t v[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const int r = min(r0 + wave_u + 4 * u, W - 1);          // (rows past the stage repeat its last one; not written)
                        v[u] = col[(unsigned)r * (unsigned)a.nx];
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const int r = r0 + wave_u + 4 * u;
                        if (r < W) S[r * W + cx] = v[u];
                    }
                }
            }
        }
    } else if (staged) {
        for (int cx0 = 0; cx0 < W; cx0 += 64)
            for (int r0 = 0; r0 < W; r0 += 64) {            // 16 rows per wavefront in flight at once
                const int cx = cx0 + lane, gx = ox + cx;
                uint32_t v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const int r = r0 + wave + 4 * u, gy = oy + r;
                    v[u] = (cx < W && r < W && gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny) ? a.st[(size_t)gy * a.nx + gx] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const int r = r0 + wave + 4 * u;
                    if (cx < W && r < W) S[r * W + cx] = v[u];
                }
            }
    }
    if (staged) {
        __syncthreads();
        // H[r][c] = max of S[r][c .. c + 2R].  A thread makes 8 adjacent outputs of a row: their windows share the columns
        // c0 + 7 .. c0 + L - 1 (one running maximum), output j adds the last 7 - j columns before and the first j columns after that
        // range -- L + 7 LDS reads for 8 outputs instead of 8 L (the passes are bound by LDS traffic: this loop was 30400 of the
        // ~37000 LDS accesses a tile costs).
        if (L >= 8) {
            for (int it = threadIdx.x; it < W * (MIS_TILE / 8); it += MIS_T) {
                const int r = it % W, c0 = (it / W) * 8;
                const uint32_t *row = S + r * W + c0;
                uint32_t lo[7], hi[7];
#pragma unroll
                for (int j = 0; j < 7; j++) { lo[j] = row[j]; hi[j] = row[L + j]; }
                uint32_t common = row[7];
#pragma unroll 4
                for (int k = 8; k < L; k++) common = max(common, row[k]);
                uint32_t o[8];
                o[7] = common;
#pragma unroll
                for (int j = 6; j >= 0; j--) o[j] = max(o[j + 1], lo[j]);           // + columns c0 + j .. c0 + 6
                uint32_t m = 0u;
#pragma unroll
                for (int j = 1; j < 8; j++) { m = max(m, hi[j - 1]); o[j] = max(o[j], m); }      // + columns c0 + L .. c0 + L + j - 1
                uint4 *dst = reinterpret_cast<uint4 *>(H + r * MIS_TILE + c0);
                dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
                dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
            }
        } else
        for (int k = threadIdx.x; k < W * MIS_TILE; k += MIS_T) {
            const uint32_t *row = &S[(k / MIS_TILE) * W + (k % MIS_TILE)];     // window = columns c .. c + 2R of the row
            uint32_t m = row[0];
#pragma unroll 8
            for (int dx = 1; dx <= 2 * R; dx++) m = max(m, row[dx]);
            H[k] = m;
        }
    }
    __syncthreads();
    for (unsigned base = 0; base < n; base += MIS_T) {
        const unsigned i = base + threadIdx.x;
        const bool valid = i < n;
        const int p = (int)next_p;
        if (base + MIS_T + threadIdx.x < n) next_p = list[base + MIS_T + threadIdx.x];
        const int xi = p % a.nx, yi = p / a.nx;
        const int lx = xi - tx * MIS_TILE, ly = yi - ty * MIS_TILE;              // interior coordinates
        bool near_accepted = false, blocked = false, gone = false, top = false;
        uint32_t sp = 0u;
        if (valid && staged) {
            sp = S[(ly + R) * W + lx + R];
            gone = sp == 0u;                                                     // rejected by a neighbour's push
            uint32_t m = 0u;
            const uint32_t *col = &H[ly * MIS_TILE + lx];                        // rows ly .. ly + 2R of H
#pragma unroll 8
            for (int dy = 0; dy <= 2 * R; dy++) m = max(m, col[dy * MIS_TILE]);
            near_accepted = (m >> 31) != 0u;
            blocked = m > sp;
            top = !gone && m == sp;              // holds the window maximum: accepted unless an equal neighbour outranks it
        } else if (valid) {
            sp = a.st[p];
            gone = sp == 0u;
            const int x0 = max(xi - R, 0), x1 = min(xi + R, a.nx - 1), y0 = max(yi - R, 0), y1 = min(yi + R, a.ny - 1);
            for (int yy = y0; yy <= y1 && !near_accepted && !gone; yy++) {
                const uint32_t *row = a.st + (size_t)yy * a.nx;
                for (int xx = x0; xx <= x1; xx++) {
                    const uint32_t sv = row[xx];
                    near_accepted |= (sv >> 31) != 0u;
                    blocked |= sv > sp || (sv == sp && (xx > xi || (xx == xi && yy > yi)));
                }
            }
        }
        const bool live = valid && !gone;
        const bool reject = live && near_accepted;
        const bool wait = live && !near_accepted && blocked;
        const bool accept = live && !near_accepted && !blocked && !top;
        const unsigned short q = (unsigned short)(ly * MIS_TILE + lx);
        if (reject) a.st[p] = 0u;
        if (top) top_local[atomicAdd(&s_top, 1u)] = q;       // decided after the loop
        if (accept) {
            a.st[p] = sp | 0x80000000u;
            acc_local[atomicAdd(&s_acc, 1u)] = q;
        }
        // the candidates that stay undecided are collected in LDS and go back to the list once this pass's accepted ones are known
        const unsigned slot = wave_compact_slot(wait, &s_cursor, lane);
        if (wait) wait_local[slot] = q;
    }
    __syncthreads();
    const unsigned ntop = s_top;
    if (ntop) {
        // equal eigenvalues inside one window are ranked by position: a wavefront per candidate scans its window for an equal
        // neighbour of higher rank (one candidate after the other with the whole workgroup, and a barrier each, before: 1.7 of
        // the 11 us a dense tile lives)
        const unsigned magic = klt_div_magic((unsigned)L);                       // w / L (L >= 3, w < L * L <= 65 * 65)
        for (unsigned e = (unsigned)wave; e < ntop; e += MIS_T / 64) {
            const int q = (int)top_local[e], lx = local_of(q).lx, ly = local_of(q).ly;
            const uint32_t sp = S[(ly + R) * W + lx + R];
            bool outranked = false;
            for (int w = lane; w < L * L; w += 64) {
                const int wy = (int)klt_div_by_magic((unsigned)w, magic), dx = w - wy * L - R, dy = wy - R;
                outranked |= S[(ly + R + dy) * W + lx + R + dx] == sp && (dx > 0 || (dx == 0 && dy > 0));
            }
            const bool any = __ballot(outranked) != 0ull;
            if (lane == 0) {
                if (any) {
                    wait_local[atomicAdd(&s_cursor, 1u)] = (unsigned short)q;
                } else {
                    a.st[cell_of_local(lx, ly)] = sp | 0x80000000u;
                    acc_local[atomicAdd(&s_acc, 1u)] = (unsigned short)q;
                }
            }
        }
        __syncthreads();
    }
    // no atomics on shared words here: a word that every workgroup increments serialises the whole launch (~90 returning
    // atomics per microsecond chip-wide).  "Something is left" is a plain store of 1; the accepted candidates go to the
    // tile's own slots and are compacted once, after the last pass.
    unsigned nacc = s_acc;
    const unsigned nwait = s_cursor;
    if (have + nacc > (unsigned)a.acc_cap) nacc = (unsigned)a.acc_cap - have;      // cannot happen (one per (R+1)^2 cells)
    // back to the list: the undecided candidates outside the squares of the candidates accepted in this pass.  (The push below
    // clears the squares in the state map; a candidate of this tile inside one used to stay listed until the next pass found it
    // gone -- after the first pass that was 85 % of the list.)
    for (unsigned i0 = 0; i0 < nwait; i0 += MIS_T) {
        const unsigned i = i0 + threadIdx.x;
        const int q = i < nwait ? (int)wait_local[i] : 0, lx = local_of(q).lx, ly = local_of(q).ly;
        bool keep = i < nwait;
        if (R > 0)
            for (unsigned k = 0; k < nacc; k++) {
                const Local acc = local_of((int)acc_local[k]);
                keep = keep && (abs(lx - acc.lx) > R || abs(ly - acc.ly) > R);
            }
        const unsigned slot = wave_compact_slot(keep, &s_left, lane);
        if (keep) list[slot] = (uint32_t)cell_of_local(lx, ly);
    }
    __syncthreads();
    const unsigned left = s_left;
    if (threadIdx.x == 0) {
        a.cnt[tile] = left;
        if (left) a.remaining[round] = 1u;
        a.acc_cnt[tile] = have + nacc;
    }
    const size_t s_base = (size_t)tile * a.acc_cap + have;
    // push: every cell within the exclusion square of a newly accepted candidate is rejected right away.  None of them
    // can be accepted (two accepted candidates never lie within each other's square), so the whole square is cleared.
    if (R > 0 && nacc) {
        const unsigned magic = klt_div_magic((unsigned)L);                       // w / L (L >= 3, w < L * L <= 65 * 65)
        for (int w = threadIdx.x; w < L * L; w += MIS_T) {
            const int wy = (int)klt_div_by_magic((unsigned)w, magic), dx = w - wy * L - R, dy = wy - R;
            if ((dx | dy) == 0) continue;
            for (unsigned k = 0; k < nacc; k++) {
                const Local acc = local_of((int)acc_local[k]);
                const int gx = tx * MIS_TILE + acc.lx + dx, gy = ty * MIS_TILE + acc.ly + dy;
                if (staged && S[(acc.ly + R + dy) * W + acc.lx + R + dx] == 0u) continue;
                if (gx >= 0 && gy >= 0 && gx < a.nx && gy < a.ny) a.st[(size_t)gy * a.nx + gx] = 0u;
            }
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < nacc; i += MIS_T) {
        const Local acc = local_of((int)acc_local[i]);
        const int xi = tx * MIS_TILE + acc.lx, yi = ty * MIS_TILE + acc.ly;
        const uint32_t sp = staged ? S[(acc.ly + R) * W + acc.lx + R] : a.st[(size_t)yi * a.nx + xi] & 0x7fffffffu;
        a.acc_keys[s_base + i] = klt_pack_key_bits(sp, cell_x(a, xi), cell_y(a, yi));
    }
}

// One workgroup = TPW consecutive tiles of its XCD's eighth (see xcd_tile), one after the other.  After the first pass most tiles have
// nothing left to decide, and a workgroup whose only act is to find that out costs a launch slot and a round trip to its counter: 6780
// such workgroups (4K) were 5-8 us of every later pass.  Four tiles per workgroup, their counters requested together, make that a
// quarter of the workgroups with one round trip each; the first pass, where almost every tile has work, keeps one tile per workgroup.
constexpr int MIS_TPW_MAX = 4;
template <int RC>
__global__ __launch_bounds__(MIS_T) void mis_round_kernel(MisArgs a, int round, int tpw)
{
    const unsigned ntile = (unsigned)(((a.nx + MIS_TILE - 1) / MIS_TILE) * ((a.ny + MIS_TILE - 1) / MIS_TILE));
    const unsigned i = blockIdx.x >> 3;
    unsigned first, len;
    xcd_range(blockIdx.x & 7u, ntile, first, len);
    unsigned cnt[MIS_TPW_MAX];
#pragma unroll
    for (int sub = 0; sub < MIS_TPW_MAX; sub++) {
        const unsigned j = i * (unsigned)tpw + (unsigned)sub;
        cnt[sub] = sub < tpw && j < len ? a.cnt[first + j] : 0u;
    }
#pragma unroll
    for (int sub = 0; sub < MIS_TPW_MAX; sub++) {
        if (cnt[sub] == 0u) continue;                                                     // (uniform: the whole workgroup skips the tile)
        mis_round_tile<RC>(a, round, first + i * (unsigned)tpw + (unsigned)sub, cnt[sub]);
        __syncthreads();
    }
}

// block-wide helpers (256 threads): sum, and inclusive scan, of one unsigned per thread
__device__ __forceinline__ unsigned block_sum_256(unsigned v, unsigned *red /* [4] */)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const unsigned t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

__device__ __forceinline__ unsigned block_scan_256(unsigned v, unsigned *red /* [4] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < wave; w++) base += red[w];
    __syncthreads();
    return base + inc;
}

// "How many before my block": thread tid's share (i = tid, tid + 256, ...) of the sum of count(load(i)) over i in [0, t0); block_sum_256
// makes the workgroup's total of it.  Sixteen loads in flight (the last workgroup of a 20 000-feature list walks 78 strides of 256
// records), then the tail as one more batch of clamped, unconditional loads (a guard is a branch).
// (mis_compact_kernel keeps its own copy: through this template, in every form tried, it takes 52 VGPRs instead of 50.)
template <class Load, class Count>
__device__ __forceinline__ unsigned count_before(int tid, int t0, Load load, Count count)
{
    unsigned before = 0;
    int i = tid;
    for (; i + 15 * 256 < t0; i += 16 * 256) {
        decltype(load(0)) v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = load(i + u * 256);
#pragma unroll
        for (int u = 0; u < 16; u++) before += count(v[u]);
    }
    decltype(load(0)) v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) v[u] = load(min(i + u * 256, max(t0 - 1, 0)));
#pragma unroll
    for (int u = 0; u < 16; u++) before += i + u * 256 < t0 ? count(v[u]) : 0u;
    return before;
}

// accepted candidates of all tiles -> one dense array (tile order) + their number.  One thread per tile, any number of
// workgroups: a workgroup first adds up the counts of the tiles before its own 256 (a few thousand words from L2), scans its
// own, and every thread copies its tile's keys.  (The single-workgroup version took 10.7 us at 1080p and 30.7 us at 4K.
// Keeping only the keys that can reach a free slot -- a histogram of the accepted keys, the bin that leaves `free slots` above
// it -- would shrink the O(n^2) ranking behind it, but building that histogram costs more than it saves: 1.4 us per pass with
// one global atomic per accepted key, 16 / 37 us with every compaction workgroup histogramming all keys in LDS.)
__global__ __launch_bounds__(256) void mis_compact_kernel(const unsigned long long *__restrict__ tile_keys, const unsigned *__restrict__ acc_cnt,
                                                          int tiles, int cap, unsigned long long *__restrict__ out, unsigned *__restrict__ out_count)
{
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, t0 = blockIdx.x * 256, t = t0 + tid;
    unsigned before = 0;
    {
        // count_before, written out.  Sixteen loads in flight: the last workgroup of a 4K frame walks 22 strides of 256 counts, and a
        // loop that waits for every load in turn made this kernel 22 us long (round-3 kernel trace) for 5 us of work
        int i = tid;
        for (; i + 15 * 256 < t0; i += 16 * 256) {
            unsigned v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) v[u] = acc_cnt[i + u * 256];
#pragma unroll
            for (int u = 0; u < 16; u++) before += v[u];
        }
        unsigned v[16];                                         // the tail: clamped, unconditional loads (a guard is a branch)
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = acc_cnt[min(i + u * 256, max(t0 - 1, 0))];
#pragma unroll
        for (int u = 0; u < 16; u++) before += i + u * 256 < t0 ? v[u] : 0u;
    }
    const unsigned base = block_sum_256(before, red);
    const unsigned c = t < tiles ? acc_cnt[t] : 0u;
    const unsigned incl = block_scan_256(c, red);
    {                                                                      // thread = tile; 8 loads in flight at a time
        const unsigned long long *src = tile_keys + (size_t)t * cap;
        unsigned long long *dst = out + base + incl - c;
        for (unsigned k0 = 0; k0 < c; k0 += 8) {
            unsigned long long v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = k0 + u < c ? src[k0 + u] : 0ull;
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (k0 + u < c) dst[k0 + u] = v[u];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 255) *out_count = base + incl;
}

// workgroup `block` of `nblocks` (256 threads each) takes its stride of the n words to clear
__device__ __forceinline__ void zero_words(unsigned *__restrict__ p, size_t n, size_t block, size_t nblocks)
{
    for (size_t i = block * 256 + threadIdx.x; i < n; i += nblocks * 256) p[i] = 0u;
}

__global__ __launch_bounds__(256) void zero_words_kernel(unsigned *__restrict__ p, size_t n) { zero_words(p, n, blockIdx.x, gridDim.x); }

// ---- placement of the accepted candidates: rank by counting, then the first `free slots` fill the list
// free slots in list order (selectGoodFeatures.py:109-110): every slot when overwriting, else the lost features
// one launch before the passes: the first workgroups list the free slots and keep a copy of the list (a repeated attempt
// starts from it), the others clear the counters
__global__ __launch_bounds__(256) void mis_prepare_kernel(const klt_feat *__restrict__ fl, int nfeat, int overwrite_all, int *__restrict__ slots,
                                                          int *__restrict__ nfill_out, klt_feat *__restrict__ snapshot,
                                                          unsigned *__restrict__ zero, size_t zero_n, int feat_blocks)
{
    if ((int)blockIdx.x >= feat_blocks) {
        zero_words(zero, zero_n, blockIdx.x - feat_blocks, gridDim.x - feat_blocks);
        return;
    }
    // workgroup b owns features [256 b, 256 b + 256): copies them, and (REPLACING_SOME) lists the lost ones among them behind
    // the lost ones of all earlier features, which it counts itself
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, f0 = blockIdx.x * 256, f = f0 + tid;
    klt_feat ft;
    ft.val = 0;
    if (f < nfeat) { ft = fl[f]; snapshot[f] = ft; }
    if (overwrite_all) { if (f == 0) *nfill_out = nfeat; return; }
    const unsigned before = count_before(tid, f0, [=](int i) { return fl[i].val; }, [](int val) { return val < 0 ? 1u : 0u; });
    const unsigned base = block_sum_256(before, red);
    const unsigned lost = (f < nfeat && ft.val < 0) ? 1u : 0u;
    const unsigned incl = block_scan_256(lost, red);
    if (lost) slots[base + incl - 1] = f;
    if ((int)blockIdx.x == feat_blocks - 1 && tid == 255) *nfill_out = (int)(base + incl);
}

// the few words the host looks at, written straight into pinned host memory: [0, look) "undecided left" flags of the
// last passes, [64, 68) prefilter info, [72] placed, [73] candidates ran out
__device__ __forceinline__ void write_results(unsigned *host_out, const unsigned *rem, int look, const unsigned *info, int placed, int ranout)
{
    for (int i = threadIdx.x; i < look; i += blockDim.x) host_out[i] = rem[i];
    if (threadIdx.x < 4) host_out[64 + threadIdx.x] = info[threadIdx.x];
    if (threadIdx.x == 0) { host_out[72] = (unsigned)placed; host_out[73] = (unsigned)ranout; }
}

__global__ void mis_results_kernel(unsigned *host_out, const unsigned *rem, int look, const unsigned *info, const int *placed)
{
    write_results(host_out, rem, look, info, placed[0], placed[1]);
}

// rank[i] = number of accepted keys greater than key i (keys are distinct).  The number of accepted keys is only known on the
// device, so the grid is fixed and every workgroup walks the (i-chunk, j-chunk) pairs with its stride: a REPLACING_SOME pass that
// accepted a few hundred candidates does one pair, where a grid sized for the worst case launched 73 000 empty workgroups at 4K.
constexpr int RANK_T = 256, RANK_GX = 96, RANK_GY = 96;
__global__ __launch_bounds__(RANK_T) void mis_rank_kernel(const unsigned long long *__restrict__ keys, const unsigned *__restrict__ count,
                                                          unsigned *__restrict__ rank)
{
    __shared__ unsigned long long other[RANK_T];
    const unsigned n = *count, nchunks = (n + RANK_T - 1) / RANK_T;
    for (unsigned ic = blockIdx.x; ic < nchunks; ic += gridDim.x) {
        const unsigned i = ic * RANK_T + threadIdx.x;
        const unsigned long long key = i < n ? keys[i] : ~0ull;
        unsigned greater = 0;
        for (unsigned jc = blockIdx.y; jc < nchunks; jc += gridDim.y) {
            __syncthreads();
            other[threadIdx.x] = jc * RANK_T + threadIdx.x < n ? keys[jc * RANK_T + threadIdx.x] : 0ull;
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < RANK_T; j++) greater += other[j] > key ? 1u : 0u;
        }
        if (i < n && greater) atomicAdd(&rank[i], greater);
    }
}

// Rank placement: accepted key i goes to the free slot of its rank.  FILTERED: the keys went through the quota filter (quota_round_kernel)
// -- the zero keys are skipped (mis_rank_kernel counted none of them as greater than anything) and *nkept keys are left.  The count
// argument is one struct per FILTERED value, so that the plain kernel receives nothing it does not read.
struct PlaceCount { const unsigned *count; };
struct PlaceCountFiltered : PlaceCount { const unsigned *nkept; };
template <bool FILTERED>
__global__ __launch_bounds__(256) void mis_place_kernel(NmsArgs a, std::conditional_t<FILTERED, PlaceCountFiltered, PlaceCount> c,
                                                        const unsigned *__restrict__ rank, const int *__restrict__ nfill_in, unsigned *host_out,
                                                        const unsigned *rem, int look, const unsigned *info)
{
    const int n = (int)*c.count, nfill = *nfill_in;
    int left = n;
    if constexpr (FILTERED) left = (int)*c.nkept;
    const int placed = min(left, nfill);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int r = (int)rank[i];
        if (r < nfill) {
            const unsigned long long k = a.keys[i];
            if (!FILTERED || k != 0ull) fill_slot(a, a.overwrite_all ? r : a.slots[r], k);
        }
    }
    if (a.overwrite_all)                                           // candidates exhausted
        for (int s = placed + i; s < a.nfeat; s += gridDim.x * 256) mark_not_found(a.fl, s);
    if (i == 0 && a.placed_out) {
        a.placed_out[0] = placed;
        a.placed_out[1] = placed < nfill ? 1 : 0;       // 1: the candidates ran out before the list was full
    }
    if (blockIdx.x == 0) write_results(host_out, rem, look, info, placed, placed < nfill ? 1 : 0);
}

__global__ void unpack_candidates_kernel(const unsigned long long *__restrict__ keys, int n, float *__restrict__ val,
                                         int *__restrict__ x, int *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    val[i] = klt_key_val(key);
    x[i] = klt_key_x(key);
    y[i] = klt_key_y(key);
}

// ------------------------------------------------------------------ per-cell quota (klt_set_select_grid)
// The members of the accepted sequence A (what the walk accepts by distance, in rank order) that are kept are the first cap(cell) of
// each cell, cap(cell) = max(q - live(cell), 0); everything else about A -- who excludes whom -- is as without a grid.  (quota_cell and
// quota_left stand in front of the walk, which uses them under a quota.)

// live(cell): list records with val >= 0 whose position lies inside the frame (f32 comparisons: a NaN fails), counted in the cell of
// ((int)x, (int)y).  A sum: the order the additions arrive in does not matter.
__global__ __launch_bounds__(256) void quota_live_kernel(const klt_feat *__restrict__ fl, int nfeat, int ncols, int nrows, QuotaArgs g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nfeat) return;
    const klt_feat ft = fl[i];
    if (ft.val < 0) return;
    if (!(ft.x >= 0.f && ft.x < (float)ncols && ft.y >= 0.f && ft.y < (float)nrows)) return;
    atomicAdd(&g.live[quota_cell(g, (int)ft.x, (int)ft.y)], 1u);
}

// The filter in front of the rank placement, one launch per round r = 0 .. q: round r < q leaves in cur[cell] the largest key of the cell
// that is below prev[cell], the largest of round r - 1 -- the cell's (r + 1)-th accepted candidate -- for every cell with r < cap(cell).
// A key that finds itself in prev[] was one of the first cap(cell) of its cell and sets bit 63 (the sign of a positive eigenvalue, never
// set in a key); round q only looks, clears the bit of the keys that have it and zeroes the others.  Maxima of distinct keys: what a round
// leaves does not depend on the order its atomics arrive in.  thr = 3 planes of ncells words: prev, cur, and the plane round r + 1
// collects in, which round r clears.
constexpr unsigned long long QUOTA_KEPT = 1ull << 63;
__global__ __launch_bounds__(256) void quota_round_kernel(unsigned long long *__restrict__ keys, const unsigned *__restrict__ count, QuotaArgs g,
                                                          unsigned long long *__restrict__ thr, int ncells, int r, unsigned *__restrict__ nkept)
{
    const unsigned long long *prev = thr + (size_t)(r % 3) * ncells;
    unsigned long long *cur = thr + (size_t)((r + 1) % 3) * ncells, *next = thr + (size_t)((r + 2) % 3) * ncells;
    const bool last = r == g.q;
    const int n = (int)*count, stride = gridDim.x * 256, first = blockIdx.x * 256 + threadIdx.x;
    if (!last)
        for (int c = first; c < ncells; c += stride) next[c] = 0ull;
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += stride) {              // (whole wavefronts stay together for the ballot below)
        const int i = i0 + threadIdx.x;
        unsigned long long k = i < n ? keys[i] : 0ull;
        if (k != 0ull && !(k & QUOTA_KEPT)) {
            const int cell = quota_cell(g, klt_key_x(k), klt_key_y(k)), cap = quota_left(g, cell);
            if (r >= 1 && r - 1 < cap && k == prev[cell]) {
                k |= QUOTA_KEPT;
                if (!last) keys[i] = k;
            } else if (!last && r < cap && (r == 0 || k < prev[cell])) {
                atomicMax(&cur[cell], k);
            }
        }
        if (last) {
            const bool kept = (k & QUOTA_KEPT) != 0ull;
            if (i < n) keys[i] = kept ? k & ~QUOTA_KEPT : 0ull;
            const unsigned long long m = __ballot(kept);
            if ((threadIdx.x & 63) == 0 && m) atomicAdd(nkept, (unsigned)__popcll(m));
        }
    }
}

}  // namespace

// a grid of `blocks` workgroups, at least one and at most `cap`
static unsigned clamp_grid(size_t blocks, unsigned cap) { return (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap); }

void launch_sat_rows(hipStream_t s, const float *gx, const float *gy, float *sat, int ncols, int nrows)
{
    hipLaunchKernelGGL(sat_rows_kernel, dim3((nrows + SR_ROWS - 1) / SR_ROWS), dim3(SR_T), 0, s, gx, gy, sat, ncols, nrows);
}

void launch_sat_cols(hipStream_t s, float *sat, int ncols, int nrows)
{
    hipLaunchKernelGGL(sat_cols_kernel, dim3((ncols + SC_COLS - 1) / SC_COLS, 3), dim3(SC_T), 0, s, sat, ncols, nrows);
}

void launch_seed_fill(hipStream_t s, const klt_feat *fl, int nfeat, uint8_t *seedmap, int ncols, int nrows, int d, uint8_t stamp)
{
    if (nfeat <= 0 || d < 0) return;
    hipLaunchKernelGGL(seed_fill_kernel, dim3(nfeat), dim3(64), 0, s, fl, nfeat, seedmap, ncols, nrows, d, stamp);
}

// mask: 16-byte aligned, n bytes; seedmap: room for n rounded up to whole 16-byte pieces
void launch_seed_mask(hipStream_t s, const uint8_t *mask, uint8_t *seedmap, size_t n, uint8_t stamp)
{
    if (n == 0) return;
    const size_t blocks = (n / 16 + 255) / 256;
    hipLaunchKernelGGL(seed_mask_kernel, dim3(clamp_grid(blocks, 2048)), dim3(256), 0, s, mask, seedmap, n, stamp);
}

void launch_eigen(hipStream_t s, const SelectArgs &a)
{
    hipLaunchKernelGGL(eigen_kernel, dim3((a.npow2 + 255) / 256), dim3(256), 0, s, a);
}

void launch_topk_prefilter(hipStream_t s, const unsigned long long *keys, int n, unsigned target, unsigned *hist,
                           unsigned *info /* [0..2] + counter at [3] */, unsigned long long *out)
{
    hipLaunchKernelGGL(key_hist_kernel, dim3(256), dim3(256), 0, s, keys, n, hist, 1);
    hipLaunchKernelGGL(key_threshold_kernel, dim3(1), dim3(1024), 0, s, hist, target, info, (const int *)nullptr, 0u);
    hipLaunchKernelGGL(key_compact_kernel, dim3(512), dim3(256), 0, s, keys, n, info, out, info + 3);
}

// threshold bin for the parallel passes from a histogram of every 4th key (counts in info[] are in sampled units)
void launch_key_threshold(hipStream_t s, const unsigned long long *keys, int n, unsigned target, unsigned *hist, unsigned *info)
{
    hipLaunchKernelGGL(key_hist_kernel, dim3(256), dim3(256), 0, s, keys, n, hist, 4);
    hipLaunchKernelGGL(key_threshold_kernel, dim3(1), dim3(1024), 0, s, hist, (target + 3u) / 4u, info, (const int *)nullptr, 0u);
}

void launch_zero_words(hipStream_t s, unsigned *p, size_t n)
{
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(zero_words_kernel, dim3(clamp_grid(blocks, 1024)), dim3(256), 0, s, p, n);
}

int mis_tiles(int nx, int ny) { return ((nx + MIS_TILE - 1) / MIS_TILE) * ((ny + MIS_TILE - 1) / MIS_TILE); }

size_t mis_stage_bytes(int R)
{
    const size_t W = MIS_TILE + 2 * (R > 0 ? R : 0);
    return R > 0 ? (W * MIS_TILE + W * W) * sizeof(uint32_t) : 0;
}

void launch_mis_init(hipStream_t s, const MisArgs &a)
{
    hipLaunchKernelGGL(mis_init_kernel, dim3(mis_tiles(a.nx, a.ny)), dim3(MIS_T), 0, s, a);
}

template <int RC>
static int launch_mis_round_t(hipStream_t s, const MisArgs &a, int round, size_t lds)
{
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)mis_round_kernel<RC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    static const int tpw_later = getenv("KLT_MIS_TPW") ? atoi(getenv("KLT_MIS_TPW")) : MIS_TPW_MAX;      // 1: every pass one tile per workgroup
    // (a selection of all features has hundreds of candidates per tile for several passes: four tiles per workgroup one after the other
    // took its 5000-feature selection at 1080p from 0.149 to 0.185 ms)
    const int tpw = round == 0 || !a.sparse ? 1 : (tpw_later < 1 ? 1 : (tpw_later > MIS_TPW_MAX ? MIS_TPW_MAX : tpw_later));
    const int tiles = mis_tiles(a.nx, a.ny), per_xcd = (tiles + 7) / 8;
    hipLaunchKernelGGL(mis_round_kernel<RC>, dim3(8 * ((per_xcd + tpw - 1) / tpw)), dim3(MIS_T), lds, s, a, round, tpw);
    return 0;
}

size_t mis_pass_lds(const MisArgs &a)
{
    return (a.stage ? mis_stage_bytes(a.R) : 0) + (((size_t)a.acc_cap * sizeof(unsigned short) + 15) & ~(size_t)15);
}

int launch_mis_round(hipStream_t s, const MisArgs &a, int round)
{
    const size_t lds = mis_pass_lds(a);
    return a.R == 9 ? launch_mis_round_t<9>(s, a, round, lds) : launch_mis_round_t<0>(s, a, round, lds);
}

void launch_mis_compact(hipStream_t s, const MisArgs &a, unsigned long long *out, unsigned *out_count)
{
    const int tiles = mis_tiles(a.nx, a.ny);
    hipLaunchKernelGGL(mis_compact_kernel, dim3((tiles + 255) / 256), dim3(256), 0, s, a.acc_keys, a.acc_cnt, tiles, a.acc_cap, out, out_count);
}

int mis_tile_capacity(int R)
{
    if (R < 0) return MIS_CAP;
    const int per_side = (MIS_TILE + R) / (R + 1);      // accepted candidates are more than R cells apart in x or in y
    return per_side * per_side < MIS_CAP ? per_side * per_side : MIS_CAP;
}

void launch_mis_prepare(hipStream_t s, const klt_feat *fl, int nfeat, int overwrite_all, int *slots, int *nfill_out, klt_feat *snapshot,
                        unsigned *zero, size_t zero_n)
{
    const size_t zb = (zero_n + 1023) / 1024;
    const int feat_blocks = nfeat > 0 ? (nfeat + 255) / 256 : 1;
    hipLaunchKernelGGL(mis_prepare_kernel, dim3(feat_blocks + clamp_grid(zb, 64)), dim3(256), 0, s, fl, nfeat, overwrite_all,
                       slots, nfill_out, snapshot, zero, zero_n, feat_blocks);
}

void launch_eigen_hist(hipStream_t s, const SelectArgs &a)
{
    const int blocks = (a.nx * a.ny + 255) / 256;
    klt_launch(eigen_hist_kernel, dim3(clamp_grid(blocks, 1024)), dim3(256), 0, s, a);
    if (a.hist) hipLaunchKernelGGL(key_threshold_kernel, dim3(1), dim3(1024), 0, s, a.hist, a.hist_target, a.info, a.hist_slots, a.hist_per_slot);
}

void launch_mask_hist(hipStream_t s, const SelectArgs &a)
{
    // a.hist_target / a.hist_per_slot arrive in units of eigen_hist_kernel's sample (every 4th block)
    constexpr unsigned scale = MASK_HIST_SAMPLE / 4;
    const int per_wg = MASK_HIST_SAMPLE * 8 * 256;
    const int blocks = (a.nx * a.ny + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(mask_hist_kernel, dim3(clamp_grid(blocks, 1024)), dim3(256), 0, s, a);
    const unsigned per_slot = (a.hist_per_slot + scale - 1) / scale;
    hipLaunchKernelGGL(key_threshold_kernel, dim3(1), dim3(1024), 0, s, a.hist, (a.hist_target + scale - 1) / scale, a.info, a.hist_slots,
                       per_slot ? per_slot : 1u);
}

void launch_mis_results(hipStream_t s, unsigned *host_out, const unsigned *rem, int look, const unsigned *info, const int *placed)
{
    hipLaunchKernelGGL(mis_results_kernel, dim3(1), dim3(64), 0, s, host_out, rem, look, info, placed);
}

// keys[0 .. *count) unsorted accepted candidates, *count <= bound; rank[] zeroed by the caller.  nkept: null, or the keys went through
// launch_quota_filter, which left *nkept of them
void launch_mis_place(hipStream_t s, const NmsArgs &a, const unsigned *count, const unsigned *nkept, unsigned *rank, const int *nfill, int bound,
                      unsigned *host_out, const unsigned *rem, int look, const unsigned *info)
{
    const int chunks = (bound + RANK_T - 1) / RANK_T;
    hipLaunchKernelGGL(mis_rank_kernel, dim3(chunks < RANK_GX ? chunks : RANK_GX, chunks < RANK_GY ? chunks : RANK_GY), dim3(RANK_T), 0, s,
                       a.keys, count, rank);
    const dim3 grid((bound + 255) / 256);
    if (nkept) hipLaunchKernelGGL(mis_place_kernel<true>, grid, dim3(256), 0, s, a, PlaceCountFiltered{{count}, nkept}, rank, nfill, host_out, rem, look, info);
    else hipLaunchKernelGGL(mis_place_kernel<false>, grid, dim3(256), 0, s, a, PlaceCount{count}, rank, nfill, host_out, rem, look, info);
}

void launch_sort_desc(hipStream_t s, unsigned long long *keys, int n)
{
    // n is a power of two >= SORT_E
    hipLaunchKernelGGL(bitonic_local_sort, dim3(n / SORT_E), dim3(SORT_T), 0, s, keys);
    for (long long k = 2LL * SORT_E; k <= n; k <<= 1) {
        for (long long j = k >> 1; j >= SORT_E; j >>= 1)
            hipLaunchKernelGGL(bitonic_global_step, dim3((n / 2 + 255) / 256), dim3(256), 0, s, keys, (int)j, (int)k, n / 2);
        hipLaunchKernelGGL(bitonic_local_merge, dim3(n / SORT_E), dim3(SORT_T), 0, s, keys, (int)k);
    }
}

template <bool QUOTA>
static int launch_walk(hipStream_t s, const NmsKernArgs<QUOTA> &a)
{
    if (a.grid_in_lds) {
        const size_t lds = (size_t)a.gw * a.gh * sizeof(uint32_t);
        hipError_t e = hipFuncSetAttribute((const void *)nms_kernel<true, QUOTA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((nms_kernel<true, QUOTA>), dim3(1), dim3(NMS_T), lds, s, a);
    } else {
        hipLaunchKernelGGL((nms_kernel<false, QUOTA>), dim3(1), dim3(NMS_T), 0, s, a);
    }
    return 0;
}

int launch_nms(hipStream_t s, const NmsArgs &a, const QuotaArgs *g)
{
    return g ? launch_walk<true>(s, NmsQuotaArgs{a, *g}) : launch_walk<false>(s, a);
}

void launch_unpack_candidates(hipStream_t s, const unsigned long long *keys, int n, float *val, int *x, int *y)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(unpack_candidates_kernel, dim3((n + 255) / 256), dim3(256), 0, s, keys, n, val, x, y);
}

void launch_quota_live(hipStream_t s, const klt_feat *fl, int nfeat, int ncols, int nrows, const QuotaArgs &g)
{
    if (nfeat <= 0) return;
    hipLaunchKernelGGL(quota_live_kernel, dim3((nfeat + 255) / 256), dim3(256), 0, s, fl, nfeat, ncols, nrows, g);
}

void launch_quota_filter(hipStream_t s, unsigned long long *keys, const unsigned *count, int bound, const QuotaArgs &g,
                         unsigned long long *thr, int ncells, unsigned *nkept)
{
    const size_t most = (size_t)(bound > ncells ? bound : ncells);
    const dim3 grid(clamp_grid((most + 255) / 256, 384));
    for (int r = 0; r <= g.q; r++) hipLaunchKernelGGL(quota_round_kernel, grid, dim3(256), 0, s, keys, count, g, thr, ncells, r, nkept);
}
