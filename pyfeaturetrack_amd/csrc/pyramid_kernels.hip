// LDS-tiled, fused pyramid-build kernels for gfx950 (the fast path; conv_kernels.hip is the generic one).
//
//   smooth_grad_kernel<TIn, true>   u8/f32 frame -> smoothed level-0 image + gradx + grady   (1 launch, was 4)
//   smooth_grad_kernel<float,false> level image   -> gradx + grady                            (1 launch, was 2)
//   pyr_reduce_kernel               level l-1 image -> level l image (smooth + subsample)      (1 launch, was 2)
//
// blockIdx.z is the frame of a batch (both frames of a pair, or all pairs of a cfg-4 shard, go through one
// launch).  Every intermediate of a tile lives in LDS; HBM sees each input once (plus halo) and each output
// once, in coalesced rows.
//
// Bit-exactness.  Every output sample is computed by the same FP64 expression, in the same
// order, as scipy's correlate1d, with the f32 rounding between the horizontal and the vertical pass.
// Fusing smoothing and differentiation needs smoothed samples *outside* the frame (scipy reflects the
// smoothed image when it differentiates it).  The tile is addressed in virtual coordinates and the raw frame
// is loaded through the reflect map R; for a symmetric tap set k and any virtual x,
//     sum_j k_j raw[R(x + j)]  ==  sum_j k_j raw[R(R(x) + j)]      (bit for bit)
// because R(-1 - t) = R(t), R(2n - 1 - t) = R(t), and scipy's symmetric loop adds the pair (x[-j] + x[j])
// commutatively before multiplying.  So the smoothed value computed at a virtual position equals the smoothed
// image at the reflected position, which is what the differentiation must see.  The host only takes this
// path when the smoothing taps are symmetric (they are Gaussians) and the tile fits in LDS.
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "klt_internal.h"

#pragma clang fp contract(off)

// tools/mb/l0_stages.hip builds this file with KLT_STAGE_CLOCKS to time the stages of one workgroup; a no-op otherwise
#ifdef KLT_STAGE_CLOCKS
__device__ long long g_stage_clk[64 * 8];
__device__ long long g_block_clk[8192 * 2];       // start / end of every workgroup, and the XCC / CU it ran on
__device__ unsigned g_block_hw[8192];
#define STAGE_MARK(n)                                                                                   \
    do {                                                                                                \
        if (threadIdx.x == 0 && blockIdx.y == 8 && blockIdx.z == 0 && blockIdx.x < 64) g_stage_clk[blockIdx.x * 8 + (n)] = wall_clock64(); \
        if (threadIdx.x == 0 && ((n) == 0 || (n) == 5)) {                                                \
            const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);         \
            if (lin < 8192) {                                                                            \
                g_block_clk[2 * lin + ((n) == 5)] = wall_clock64();                                      \
                unsigned hw, xcc;                                                                        \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                         \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                       \
                g_block_hw[lin] = (hw & 0xffff) | (xcc << 16);                                           \
            }                                                                                            \
        }                                                                                                \
    } while (0)
// streaming kernel: ticks of each stage summed over the bands of segment 1 of frame 0 (stage 0 includes the barrier after the previous
// band's stage 4)
__device__ long long g_stream_clk[64 * 8];
#define STREAM_CLK_START long long stream_t_ = wall_clock64()
#define STREAM_MARK(n)                                                                                  \
    do {                                                                                                \
        if (threadIdx.x == 0 && blockIdx.y == 1 && blockIdx.z == 0 && blockIdx.x < 64) {               \
            const long long now_ = wall_clock64();                                                      \
            g_stream_clk[blockIdx.x * 8 + (n)] += now_ - stream_t_;                                     \
            stream_t_ = now_;                                                                           \
        }                                                                                               \
    } while (0)
#else
#define STAGE_MARK(n) do { } while (0)
#define STREAM_CLK_START do { } while (0)
#define STREAM_MARK(n) do { } while (0)
#endif

namespace {

constexpr int TW = 64, TH = 16;        // output tile of smooth_grad_kernel
constexpr int OW = 32, OH = 8;         // output tile of pyr_reduce_kernel
}
constexpr int OW_DEFAULT = 32, OH_DEFAULT = 8;
namespace {

__device__ __forceinline__ int reflect_idx(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// correlate1d at `c` (centre sample) of a fully populated LDS line with element stride `stride`
__device__ __forceinline__ float correlate_lds(const float *c, int stride, const Taps &t)
{
    const int size1 = t.n / 2;
    const int size2 = t.n - size1 - 1;
    const double *fw = t.k + size1;
    double acc;
    if (t.sym > 0) {
        acc = (double)c[0] * fw[0];
        for (int jj = -size1; jj < 0; jj++) acc = acc + ((double)c[jj * stride] + (double)c[-jj * stride]) * fw[jj];
    } else if (t.sym < 0) {
        acc = (double)c[0] * fw[0];
        for (int jj = -size1; jj < 0; jj++) acc = acc + ((double)c[jj * stride] - (double)c[-jj * stride]) * fw[jj];
    } else {
        acc = (double)c[size2 * stride] * fw[size2];
        for (int jj = -size1; jj < size2; jj++) acc = acc + (double)c[jj * stride] * fw[jj];
    }
    return (float)acc;
}

// ------------------------------------------------------------------------------------------------------
// frame -> [smoothed image] + gradx + grady.  grid = (ceil(ncols/TW), ceil(nrows/TH), batch), block = 256
template <typename TIn, bool SMOOTH>
__global__ __launch_bounds__(256) void smooth_grad_kernel(SmoothGradArgs a)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int nc = a.ncols, nr = a.nrows;
    const int rs = SMOOTH ? a.smooth.n / 2 : 0;
    const int R = a.R;                                   // halo of the image tile = max gradient tap radius
    const int IW = TW + 2 * R, IH = TH + 2 * R;          // image tile
    const int RW = IW + 2 * rs, RH = IH + 2 * rs;        // raw tile
    // LDS carve: [A raw RH*RW][B hsmooth RH*IW] overlaid later by [D IH*TW][E IH*TW]; then [C image IH*IW]
    const int ab = SMOOTH ? RH * RW + RH * IW : 0, de = 2 * IH * TW;
    float *A = lds, *B = lds + RH * RW, *D = lds, *E = lds + IH * TW;
    float *C = lds + (ab > de ? ab : de);
    const TIn *__restrict__ raw = (const TIn *)a.raw[b];

    if (SMOOTH) {
        for (int i = tid; i < RH * RW; i += 256) {
            const int r = i / RW, c = i - r * RW;
            const int gy = reflect_idx(ty0 - R - rs + r, nr), gx = reflect_idx(tx0 - R - rs + c, nc);
            A[i] = (float)raw[(size_t)gy * nc + gx];
        }
        __syncthreads();
        for (int i = tid; i < RH * IW; i += 256) {       // horizontal smoothing
            const int r = i / IW, c = i - r * IW;
            B[i] = correlate_lds(A + r * RW + c + rs, 1, a.smooth);
        }
        __syncthreads();
        float *__restrict__ img = a.cimg[b];             // the optional compact copy (the records get the image below)
        for (int i = tid; i < IH * IW; i += 256) {       // vertical smoothing -> image tile (+ store the interior)
            const int r = i / IW, c = i - r * IW;
            const float v = correlate_lds(B + (r + rs) * IW + c, IW, a.smooth);
            C[i] = v;
            const int y = ty0 - R + r, x = tx0 - R + c;
            if (img && r >= R && r < R + TH && c >= R && c < R + TW && y < nr && x < nc) img[(size_t)y * nc + x] = v;
        }
    } else {
        for (int i = tid; i < IH * IW; i += 256) {
            const int r = i / IW, c = i - r * IW;
            const int gy = reflect_idx(ty0 - R + r, nr), gx = reflect_idx(tx0 - R + c, nc);
            C[i] = (float)raw[(size_t)gy * nc + gx];
        }
    }
    __syncthreads();
    for (int i = tid; i < IH * TW; i += 256) {           // horizontal pass of both gradients
        const int r = i / TW, x = i - r * TW;
        const float *c = C + r * IW + x + R;
        D[i] = correlate_lds(c, 1, a.gderiv);            // gradx: derivative taps along x
        E[i] = correlate_lds(c, 1, a.ggauss);            // grady: Gaussian taps along x
    }
    __syncthreads();
    float *__restrict__ rec = a.rec[b];
    for (int i = tid; i < TH * TW; i += 256) {           // vertical pass -> the pixel records (image copied from the tile)
        const int r = i / TW, x = i - r * TW;
        const int y = ty0 + r, xx = tx0 + x;
        if (y < nr && xx < nc) {
            const size_t o = ((size_t)y * nc + xx) * KLT_PIX_STRIDE;
            rec[o] = C[(r + R) * IW + x + R];
            rec[o + 1] = correlate_lds(D + (r + R) * TW + x, TW, a.ggauss);
            rec[o + 2] = correlate_lds(E + (r + R) * TW + x, TW, a.gderiv);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// level l-1 image -> level l image: out(ys, xs) = V(H(src))(ss*ys + ss/2, ss*xs + ss/2)  (pyramid.py:59-72).
// Only the surviving columns are smoothed horizontally and only the surviving rows vertically.
// The source tile is stored de-interleaved by column phase (col % ss) so that lanes reading columns
// ss apart hit consecutive LDS addresses.  grid = (ceil(dc/OW), ceil(dr/OH), batch), block = 256
__global__ __launch_bounds__(256) void pyr_reduce_kernel(PyrReduceArgs a)
{
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int ss = a.ss, r = a.taps.n / 2;
    const int SW = (OW - 1) * ss + 2 * r + 1, SH = (OH - 1) * ss + 2 * r + 1;
    const int PW = (SW + ss - 1) / ss;                   // entries per phase plane per row
    const int rowlen = PW * ss;
    float *S = lds;                                      // SH rows x ss planes x PW
    float *Hh = lds + SH * rowlen;                       // SH x OW
    const int xs0 = blockIdx.x * OW, ys0 = blockIdx.y * OH;
    const int gx0 = xs0 * ss + ss / 2 - r, gy0 = ys0 * ss + ss / 2 - r;   // source coords of tile element (0,0)
    const float *__restrict__ src = a.src[b];
    const int nc = a.src_nc, nr = a.src_nr;

    for (int i = tid; i < SH * SW; i += 256) {
        const int rr = i / SW, c = i - rr * SW;
        const int gy = reflect_idx(gy0 + rr, nr), gx = reflect_idx(gx0 + c, nc);
        S[rr * rowlen + (c & (ss - 1)) * PW + (c >> a.log2ss)] = src[(size_t)gy * nc + gx];
    }
    __syncthreads();
    const int size1 = a.taps.n / 2, size2 = a.taps.n - size1 - 1;
    const double *fw = a.taps.k + size1;
    for (int i = tid; i < SH * OW; i += 256) {           // horizontal pass at the surviving columns
        const int rr = i / OW, xs = i - rr * OW;
        const float *row = S + rr * rowlen;
        const int cc = xs * ss + r;                      // tile column of the centre sample
        auto at = [&](int j) -> double { const int c = cc + j; return (double)row[(c & (ss - 1)) * PW + (c >> a.log2ss)]; };
        double acc;
        if (a.taps.sym > 0) {
            acc = at(0) * fw[0];
            for (int jj = -size1; jj < 0; jj++) acc = acc + (at(jj) + at(-jj)) * fw[jj];
        } else if (a.taps.sym < 0) {
            acc = at(0) * fw[0];
            for (int jj = -size1; jj < 0; jj++) acc = acc + (at(jj) - at(-jj)) * fw[jj];
        } else {
            acc = at(size2) * fw[size2];
            for (int jj = -size1; jj < size2; jj++) acc = acc + at(jj) * fw[jj];
        }
        Hh[i] = (float)acc;
    }
    __syncthreads();
    const int xs = tid % OW, ys = tid / OW;              // vertical pass at the surviving rows, one output per thread
    const int ox = xs0 + xs, oy = ys0 + ys;
    if (ox < a.dst_nc && oy < a.dst_nr)
        a.dst[b][(size_t)oy * a.dst_nc + ox] = correlate_lds(Hh + (ys * ss + r) * OW + xs, OW, a.taps);
}

// ======================================================================================================
// Compile-time specialisations.  Tap counts, tile geometry and every LDS offset are constants, the taps sit
// in scalar registers for the whole kernel and the correlate loops are fully unrolled (same operation order).
// The runtime-sized kernels above remain the fallback for unusual sigmas.


__device__ __forceinline__ int reflect_fast(int i, int n)
{
    i = reflect_once(i, n);
    if ((unsigned)i >= (unsigned)n) i = reflect_idx(i, n);      // frames smaller than the halo
    return i;
}


template <int NT>
__device__ __forceinline__ void load_taps(TapRegs<NT> &r, const Taps &t)
{
#pragma unroll
    for (int i = 0; i < NT; i++) r.k[i] = t.k[i];
}

// (corr_regs, the per-output expression of the register-blocked kernels, and reflect_once live in klt_internal.h: the tracker's level-0
// gradients on demand use the same text)

// Three aligned quads of an LDS row, widened.  The loads are volatile so that they stay three ds_read_b128: when only 8 or
// 10 of the 12 samples are used the compiler otherwise narrows them to ds_read2_b32 pairs, and dword reads at a lane stride
// of 16 bytes are 4-way bank conflicts.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void widen12(const float *row, double *d)
{
    typedef const volatile __attribute__((address_space(3))) f32x4 *lds_quad_ptr;
    const lds_quad_ptr p = (lds_quad_ptr)row;
    const f32x4 a = p[0], b = p[1], c = p[2];
    d[0] = (double)a.x; d[1] = (double)a.y; d[2] = (double)a.z; d[3] = (double)a.w;
    d[4] = (double)b.x; d[5] = (double)b.y; d[6] = (double)b.z; d[7] = (double)b.w;
    d[8] = (double)c.x; d[9] = (double)c.y; d[10] = (double)c.z; d[11] = (double)c.w;
}

// The pixel records of two horizontally adjacent pixels at byte offset `ob` (8-byte aligned): image, gradx, grady of the first, then
// of the second (`second` = false: the first only)
__device__ __forceinline__ void store_records(plane_rsrc r, unsigned ob, float2 im, float2 gx, float2 gy, bool second)
{
    float2 p;
    p.x = im.x; p.y = gx.x;
    plane_store2(r, ob, p);
    if (second) {
        p.x = gy.x; p.y = im.y;
        plane_store2(r, ob + 8, p);
        p.x = gx.y; p.y = gy.y;
        plane_store2(r, ob + 16, p);
    } else {
        plane_store(r, ob + 8, gy.x);
    }
}

// ------------------------------------------------------------------------------------------------------
// Stage primitives of the two level-0 kernels (smooth_grad_rb and smooth_grad_stream): one thread's work item of a stage, on the LDS
// pointers it is given.  The kernels keep what differs between them: the work-item loops and their thread rotation, the rows and columns
// an item maps to, the barriers, the carries between bands, the store predicates and the stage marks.

__device__ __forceinline__ float4 unpack_u8x4(uint32_t w)
{
    float4 v;
    v.x = (float)(w & 0xffu); v.y = (float)((w >> 8) & 0xffu);
    v.z = (float)((w >> 16) & 0xffu); v.w = (float)(w >> 24);
    return v;
}

// Four adjacent raw samples in registers: the packed word of a u8 frame (the streaming kernel keeps a band of them in flight in three
// registers), a float4 of an f32 frame
template <typename TIn> struct RawQuad;
template <> struct RawQuad<uint8_t> { typedef uint32_t reg; };
template <> struct RawQuad<float> { typedef float4 reg; };
__device__ __forceinline__ float4 quad_f32(uint32_t w) { return unpack_u8x4(w); }
__device__ __forceinline__ float4 quad_f32(float4 v) { return v; }

// Is the block of H rows x WQ quads at frame position (y0, x0) inside the frame, its quads aligned (raw_quads_aligned, l0_plan.h: by the
// frame's own address, which for an adopted frame is any byte)?  Workgroup-uniform scalar work.
template <int H, int WQ, typename TIn>
__device__ __forceinline__ bool raw_block_interior(const TIn *raw, int nc, int nr, int y0, int x0)
{
    return raw_quads_aligned(reinterpret_cast<uintptr_t>(raw), nc, (int)sizeof(TIn)) && x0 >= 0 && x0 + 4 * WQ <= nc && y0 >= 0 && y0 + H <= nr;
}

// Stage 0: the raw block of H rows x WQ quads at frame position (y0, x0) -> registers; w[u] = quad tid + u NTHR of the block, row-major
// (clamped: the last threads repeat the last quad).  Converting to f32 and storing to LDS is the caller's.  The frame must be large
// enough that one reflection brings every index of the block inside.
// QUADS: who has asked raw_quads_aligned about the frame's address.  BY_ADDRESS: nobody, the block asks (the tiled kernels: once per
// workgroup).  ADDRESS_TESTED / NEVER: the streaming kernels, which ask once per workgroup in front of their band loop and fold the
// answer into their EDGE instantiation (smooth_grad_stream): its blocks read element by element whatever the frame, the others'
// by the width and the block's position alone -- no address bits are held across the bands.
enum { RAW_QUADS_NEVER, RAW_QUADS_ADDRESS_TESTED, RAW_QUADS_BY_ADDRESS };
template <typename TIn, int H, int WQ, int NTHR, int QUADS = RAW_QUADS_BY_ADDRESS>
__device__ __forceinline__ void load_raw_block(const TIn *raw, int nc, int nr, int y0, int x0, int tid,
                                               typename RawQuad<TIn>::reg (&w)[(H * WQ + NTHR - 1) / NTHR])
{
    constexpr int N0 = H * WQ, U0 = (N0 + NTHR - 1) / NTHR;
    if (QUADS != RAW_QUADS_NEVER && raw_block_interior<H, WQ>(QUADS == RAW_QUADS_BY_ADDRESS ? raw : (const TIn *)nullptr, nc, nr, y0, x0)) {
        // Blocks inside the frame (most of them): every load of the thread is issued before the first one is used.  A loop
        // that waits for each of its 3-4 loads in turn costs 2.2 of the 9 us a workgroup of the tiled kernel lives.
        const plane_rsrc rawp = plane_of(raw);
        const unsigned row_b = (unsigned)nc * (unsigned)sizeof(TIn), raw_b0 = (unsigned)y0 * row_b + (unsigned)x0 * (unsigned)sizeof(TIn);
#pragma unroll
        for (int u = 0; u < U0; u++) {
            const int i = N0 % NTHR ? min(tid + u * NTHR, N0 - 1) : tid + u * NTHR;
            const unsigned off = raw_b0 + __umul24((unsigned)(i / WQ), row_b) + 4u * (unsigned)sizeof(TIn) * (unsigned)(i % WQ);
            if constexpr (sizeof(TIn) == 1) {
                w[u] = __builtin_amdgcn_raw_buffer_load_b32(rawp, off, 0, 0);
            } else {
                w[u] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rawp, off, 0, 0));
            }
        }
    } else {
        // blocks at the frame's edges: branch-free index map, all element loads of the thread in flight together
        TIn e[U0][4];
#pragma unroll
        for (int u = 0; u < U0; u++) {
            const int i = N0 % NTHR ? min(tid + u * NTHR, N0 - 1) : tid + u * NTHR;
            const TIn *row = raw + (size_t)reflect_once(y0 + i / WQ, nr) * nc;
            const int x = x0 + 4 * (i % WQ);
#pragma unroll
            for (int k = 0; k < 4; k++) e[u][k] = row[reflect_once(x + k, nc)];
        }
#pragma unroll
        for (int u = 0; u < U0; u++) {
            if constexpr (sizeof(TIn) == 1) {
                w[u] = e[u][0] | (uint32_t)e[u][1] << 8 | (uint32_t)e[u][2] << 16 | (uint32_t)e[u][3] << 24;
            } else {
                w[u].x = e[u][0]; w[u].y = e[u][1]; w[u].z = e[u][2]; w[u].w = e[u][3];
            }
        }
    }
}

// Four adjacent outputs of a horizontal pass from the twelve widened samples of their row (the outputs sit at v[4..7])
template <int NT, int SYM, bool ZC = false>
__device__ __forceinline__ float4 corr_quad(const double *v, const TapRegs<NT> &t)
{
    float4 o;
    o.x = corr_regs<NT, SYM, ZC>(v + 4, t); o.y = corr_regs<NT, SYM, ZC>(v + 5, t);
    o.z = corr_regs<NT, SYM, ZC>(v + 6, t); o.w = corr_regs<NT, SYM, ZC>(v + 7, t);
    return o;
}

// Stage 1: horizontal smoothing of the four samples that start at a[4] (a: a quad of an A row)
template <int NS>
__device__ __forceinline__ float4 hsmooth_quad(const float *a, const TapRegs<NS> &ks)
{
    double v[12];
    widen12(a, v);
    return corr_quad<NS, 1>(v, ks);
}

// Stage 3: horizontal pass of both gradients at the four samples that start at c[4] (c: a quad of a C row): d = derivative taps
// along x (gradx after stage 4), e = Gaussian taps along x (grady)
template <int NG, int ND, bool ZC>
__device__ __forceinline__ void hgrad_quad(const float *c, const TapRegs<NG> &kg, const TapRegs<ND> &kd, float4 &d, float4 &e)
{
    double v[12];
    widen12(c, v);
    d = corr_quad<ND, -1, ZC>(v, kd);
    e = corr_quad<NG, 1>(v, kg);
}

// Stage 3b: horizontal pass of the first pyramid reduction (pyramid.py:59-72 -> correlate1d along x, symmetric branch; f32 result, as
// between the reference's two passes) at TWO adjacent surviving columns (four samples apart): their 21-sample windows share 17 samples, so
// 28 samples are read and widened for two outputs instead of 24 for each.  c: the quad of a C row that starts at the first output's
// leftmost sample.  kr.k[0..NR/2]: the taps left of and at the centre (symmetric).
template <int NR>
__device__ __forceinline__ void hreduce_pair(const float *c, const TapRegs<NR / 2 + 1> &kr, float (&o)[2])
{
    constexpr int HR = NR / 2;
    static_assert(2 * HR + 4 < 28, "both windows inside the seven quads");
    typedef const volatile __attribute__((address_space(3))) f32x4 *lds_quad_ptr;      // (volatile: as in widen12)
    const lds_quad_ptr p = (lds_quad_ptr)c;
    double v[28];
#pragma unroll
    for (int u = 0; u < 7; u++) {
        const f32x4 t = p[u];
        v[4 * u] = (double)t.x; v[4 * u + 1] = (double)t.y; v[4 * u + 2] = (double)t.z; v[4 * u + 3] = (double)t.w;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const double *m = v + HR + 4 * i;                        // centre sample of output i
        double acc = m[0] * kr.k[HR];
#pragma unroll
        for (int jj = -HR; jj < 0; jj++) acc = acc + (m[jj] + m[-jj]) * kr.k[HR + jj];
        o[i] = (float)acc;
    }
}

// The vertical passes (stages 2 and 4).  A thread makes two adjacent columns on FOUR consecutive rows: the NT + 3 rows of two samples
// they need are read (ds_read_b64) and widened once for 8 outputs -- with 7 taps 2.5 widenings per output where a quad on two rows
// needs 4, with 5 taps 2 against 3 (the widening is an FP64-rate instruction like the adds and multiplies).
// p: the two samples of the first row, rows STRIDE floats apart; rows past jlast are read as row jlast (they only feed outputs that
// the caller does not make).
template <int NROWS, int STRIDE>
__device__ __forceinline__ void widen_col_pair(const float *p, int jlast, double (&v)[2][NROWS])
{
#pragma unroll
    for (int j = 0; j < NROWS; j++) {
        const float2 t = *reinterpret_cast<const float2 *>(p + min(j, jlast) * STRIDE);
        v[0][j] = (double)t.x; v[1][j] = (double)t.y;
    }
}

// ... and output row dr (0..3) of the two columns
template <int NT, int SYM, bool ZC = false>
__device__ __forceinline__ float2 corr_pair(const double (&v)[2][NT + 3], int dr, const TapRegs<NT> &t)
{
    float2 o;
    o.x = corr_regs<NT, SYM, ZC>(v[0] + NT / 2 + dr, t); o.y = corr_regs<NT, SYM, ZC>(v[1] + NT / 2 + dr, t);
    return o;
}

// Stage 4: vertical pass of both gradients, two columns x four rows: D -> gradx (Gaussian taps), E -> grady (derivative taps).
// d, e: the two samples of the first of the NG + 3 rows of D and of E.
template <int NG, int ND, int STRIDE, bool ZC>
__device__ __forceinline__ void vgrad_2x4(const float *d, const float *e, const TapRegs<NG> &kg, const TapRegs<ND> &kd, float2 (&ox)[4], float2 (&oy)[4])
{
    {
        double v[2][NG + 3];
        widen_col_pair<NG + 3, STRIDE>(d, NG + 2, v);
#pragma unroll
        for (int dr = 0; dr < 4; dr++) ox[dr] = corr_pair<NG, 1>(v, dr, kg);
    }
    {
        double v[2][ND + 3];
        widen_col_pair<ND + 3, STRIDE>(e, ND + 2, v);
#pragma unroll
        for (int dr = 0; dr < 4; dr++) oy[dr] = corr_pair<ND, -1, ZC>(v, dr, kd);
    }
}

#ifndef KLT_L0_WAVES
#define KLT_L0_WAVES 4
#endif
// HRED: the kernel also runs the HORIZONTAL pass of the first pyramid reduction (subsampling 4, 21 taps) on the smoothed tile while it
// is in LDS, and writes H1[y][x] = hsmooth(image)(y, 4x + 2) (f32, nrows x ncols/4); pyr_vreduce_kernel finishes level 1 from
// H1.  The image tile carries a halo of 12 columns instead of 4 for that (+22 % smoothing work in this kernel), and the separate
// reduction kernel -- with its halo re-reads of the level-0 image, its 1.6x redundant horizontal pass and its latency-bound
// tile loads -- disappears for level 1.  Same values: the tile is addressed in virtual coordinates whose smoothed values equal
// the reflected ones (header of this file), which is what the reference's reduction reads beyond the frame edge.
// EDGE = false: the instantiation for tiles whose outputs all land inside the frame (every tile but the last row / column of tiles of
// a frame whose size is not a multiple of the tile): the per-row and per-column store predicates fold away.
// LDS layout of the tiled kernel: floats per row, rows and region sizes, for the kernel (array size) and the tile body (offsets)
template <bool SMOOTH, int NS, int NG, int ND, int TH_, bool HRED>
struct TileLds {
    static_assert(!HRED || SMOOTH, "the fused horizontal reduction needs the smoothing stages");
    static constexpr int HB = HRED ? 12 : 4;                    // halo columns of the image tile (B, C) on each side
    static constexpr int rs = SMOOTH ? NS / 2 : 0, R = (NG > ND ? NG : ND) / 2;
    static_assert(rs <= 4 && R <= 4, "register-blocked kernel needs tap radii <= 4");
    static constexpr int AW = TW + 2 * HB + 8, BW = TW + 2 * HB, DW = TW;   // floats per row (A starts at column -HB-4, B / C at -HB, D / E at 0)
    static constexpr int IH = TH_ + 2 * R, RH = IH + 2 * rs;
    // LDS regions.  With smoothing: [A | C] then [B | D E] -- the raw tile A is dead once B exists and the smoothed tile C takes its
    // place; B is dead once C exists and the two gradient intermediates D, E take its place (they are written while C is read,
    // so they cannot share C's region).  35.6 KB for the 32-row tile with the fused reduction: four workgroups per CU, and the
    // 2040 tiles of a 1080p pair are two full rounds of the 1024 slots (44 KB / three per CU before: 2.66 rounds).
    // Without smoothing (gradients of levels >= 1): C, then D E.
    static constexpr int AC = SMOOTH ? (RH * AW > IH * BW ? RH * AW : IH * BW) : IH * BW;
    static constexpr int BDE = SMOOTH ? (RH * BW > 2 * IH * DW ? RH * BW : 2 * IH * DW) : 2 * IH * DW;
    static constexpr int total = AC + BDE;
};

template <typename TIn, bool SMOOTH, int NS, int NG, int ND, int TH_, int NTHR, bool HRED, bool EDGE>
__device__ __forceinline__ void smooth_grad_rb_tile(const SmoothGradArgs &a, float *const lds, const int nc, const int nr)
{
    using L = TileLds<SMOOTH, NS, NG, ND, TH_, HRED>;
    constexpr int HB = L::HB, rs = L::rs, R = L::R, AW = L::AW, BW = L::BW, DW = L::DW, IH = L::IH, RH = L::RH;
    constexpr int AQ = AW / 4, BQ = BW / 4, DQ = DW / 4;        // quads per row
    float *const A = lds, *const C = lds, *const B = lds + L::AC, *const D = lds + L::AC, *const E = lds + L::AC + IH * DW;
    const int tid = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH_;
    // two adjacent outputs of the compact image copy go out as one 8-byte store where every row keeps them aligned (block-uniform)
    const bool vec2_ok = (nc & 1) == 0 && (reinterpret_cast<uintptr_t>(a.cimg[b]) & 7) == 0;
    const TIn *__restrict__ raw = (const TIn *)a.raw[b];
    const unsigned row_bytes = 4u * (unsigned)nc;                // of the f32 planes
    const unsigned tile_b0 = (unsigned)ty0 * row_bytes + 4u * (unsigned)tx0;   // byte offset of the tile's first output in them
    TapRegs<NG> kg;
    TapRegs<ND> kd;
    load_taps(kg, a.ggauss);
    load_taps(kd, a.gderiv);

    STAGE_MARK(0);
    // ---- stage 0: frame -> LDS (through the reflect map)
    {
        constexpr int W0 = SMOOTH ? AQ : BQ, H0 = SMOOTH ? RH : IH, X0 = SMOOTH ? -(HB + 4) : -HB, Y0 = -(R + rs);
        float *const dst = SMOOTH ? A : C;
        constexpr int N0 = H0 * W0, U0 = (N0 + NTHR - 1) / NTHR;
        const bool quads = raw_quads_aligned(reinterpret_cast<uintptr_t>(raw), nc, (int)sizeof(TIn));   // block-uniform, outside the loops
        // tiles whose halo lies inside the frame, and frame-edge tiles of frames large enough that one reflection brings every index inside
        if (raw_block_interior<H0, W0>(raw, nc, nr, ty0 + Y0, tx0 + X0) || (nc >= 2 * TW && nr >= 2 * TH_)) {
            typename RawQuad<TIn>::reg w[U0];
            load_raw_block<TIn, H0, W0, NTHR>(raw, nc, nr, ty0 + Y0, tx0 + X0, tid, w);
#pragma unroll
            for (int u = 0; u < U0; u++) {
                const int i = tid + u * NTHR;
                if (i < N0) *reinterpret_cast<float4 *>(dst + (size_t)i * 4) = quad_f32(w[u]);
            }
        } else
        for (int i = tid; i < H0 * W0; i += NTHR) {              // frames smaller than the halo
            const int r = i / W0, q = i % W0;
            const int gy = reflect_fast(ty0 + Y0 + r, nr);
            const int x = tx0 + X0 + 4 * q;
            const TIn *row = raw + (size_t)gy * nc;
            float4 v;
            if (quads && x >= 0 && x + 3 < nc) {                  // aligned quad: one 4- or 16-byte load
                if constexpr (sizeof(TIn) == 1) v = unpack_u8x4(*reinterpret_cast<const uint32_t *>(row + x));
                else v = *reinterpret_cast<const float4 *>(row + x);
            } else if (x >= 0 && x + 3 < nc) {
                v.x = (float)row[x]; v.y = (float)row[x + 1]; v.z = (float)row[x + 2]; v.w = (float)row[x + 3];
            } else {
                v.x = (float)row[reflect_fast(x, nc)]; v.y = (float)row[reflect_fast(x + 1, nc)];
                v.z = (float)row[reflect_fast(x + 2, nc)]; v.w = (float)row[reflect_fast(x + 3, nc)];
            }
            *reinterpret_cast<float4 *>(dst + (size_t)i * 4) = v;
        }
    }
    __syncthreads();
    STAGE_MARK(1);
    if (SMOOTH) {
        TapRegs<NS> ks;
        load_taps(ks, a.smooth);
        // ---- stage 1: horizontal smoothing, A -> B (B column c = A column c + 4)
        for (int i = tid; i < RH * BQ; i += NTHR) {
            const int r = i / BQ, q = i % BQ;
            *reinterpret_cast<float4 *>(B + r * BW + 4 * q) = hsmooth_quad<NS>(A + r * AW + 4 * q, ks);
        }
        __syncthreads();
        STAGE_MARK(2);
        // ---- stage 2: vertical smoothing, B -> C (+ store the tile interior of the compact image copy, if one is asked for; the
        // records take the image from C in stage 4)
        const bool cimg_out = a.cimg[b] != nullptr;
        const plane_rsrc img = plane_of(a.cimg[b]);
        constexpr int BH = BW / 2, G2 = (IH + 3) / 4;           // half-quads per row, groups of four rows (the last one may be partial)
        for (int i = tid; i < G2 * BH; i += NTHR) {
            const int r = 4 * (i / BH), h = i % BH;
            // byte offset of (ty0 - R + r, tx0 - HB + 2 h) modulo 2^32 (rows above the frame are never stored)
            const unsigned img_b0 = tile_b0 + __umul24((unsigned)r, row_bytes) - (unsigned)R * row_bytes + (unsigned)(8 * h) - (unsigned)(4 * HB);
            double v[2][NS + 3];
            widen_col_pair<NS + 3, BW>(B + r * BW + 2 * h, RH - 1 - r, v);
#pragma unroll
            for (int dr = 0; dr < 4; dr++) {
                const int rr = r + dr;
                if (rr >= IH) break;
                const float2 o = corr_pair<NS, 1>(v, dr, ks);
                *reinterpret_cast<float2 *>(C + rr * BW + 2 * h) = o;
                const int y = ty0 - R + rr, x = tx0 - HB + 2 * h;
                if (cimg_out && rr >= R && rr < R + TH_ && h >= HB / 2 && h < HB / 2 + DW / 2 && (!EDGE || y < nr)) {
                    const unsigned ob = img_b0 + (unsigned)dr * row_bytes;          // byte offset of (y, x)
                    if (!EDGE && vec2_ok) plane_store2(img, ob, o);                  // x is even
                    else if (!EDGE) { plane_store(img, ob, o.x); plane_store(img, ob + 4, o.y); }
                    else {
                        if (x < nc) plane_store(img, ob, o.x);
                        if (x + 1 < nc) plane_store(img, ob + 4, o.y);
                    }
                }
            }
        }
        __syncthreads();
    }
    STAGE_MARK(3);
    // ---- stage 3: horizontal pass of both gradients, C -> D (derivative taps), E (Gaussian taps)
    // (the partial last round of this loop goes to wavefronts 2 and 3: stage 2 gave its partial round to wavefronts 0
    // and 1, and wavefront w of every workgroup of a CU sits on SIMD w -- the rotation evens out the SIMDs)
    for (int i = (tid + NTHR / 2) & (NTHR - 1); i < IH * DQ; i += NTHR) {
        const int r = i / DQ, q = i % DQ;
        float4 d, e;
        hgrad_quad<NG, ND, false>(C + r * BW + 4 * q + (HB - 4), kg, kd, d, e);
        *reinterpret_cast<float4 *>(D + r * DW + 4 * q) = d;
        *reinterpret_cast<float4 *>(E + r * DW + 4 * q) = e;
    }
    if (HRED) {
        // ---- stage 3b: horizontal pass of the pyramid reduction at the surviving columns 4x + 2 of the tile's own rows
        constexpr int NR = 21, HR = NR / 2;
        TapRegs<HR + 1> kr;
#pragma unroll
        for (int t = 0; t <= HR; t++) kr.k[t] = a.reduce.k[t];
        const plane_rsrc h1 = plane_of(a.h1[b]);
        const int h1_nc = a.h1_nc;
        const unsigned h1_row_bytes = 4u * (unsigned)h1_nc, h1_b0 = (unsigned)ty0 * h1_row_bytes + (unsigned)tx0;   // (ty0, tx0 / 4); tx0 % 4 == 0
        static_assert(DQ % 2 == 0, "tile width must be a multiple of eight");
        for (int i = tid; i < TH_ * (DQ / 2); i += NTHR) {
            const int r = i / (DQ / 2), xs = 2 * (i % (DQ / 2));     // outputs at columns 4 xs + 2 and 4 xs + 6 of the tile
            // centre = image column 4 xs + 2 = C index HB + 4 xs + 2; samples -10 .. +10 start at C index 4 xs + HB - 8 (a quad)
            float o[2];
            hreduce_pair<NR>(C + (r + R) * BW + 4 * xs + (HB - 8), kr, o);
            const int y = ty0 + r;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int xg = tx0 / 4 + xs + k;
                if (!EDGE || (y < nr && xg < h1_nc))
                    plane_store(h1, h1_b0 + __umul24((unsigned)r, h1_row_bytes) + 4u * (unsigned)(xs + k), o[k]);
            }
        }
    }
    __syncthreads();
    STAGE_MARK(4);
    // ---- stage 4: vertical pass, D -> gradx, E -> grady.  The two pixel records (image from C, gradx, grady) of a row go out
    // together: 24 contiguous bytes.
    const plane_rsrc recp = plane_of(a.rec[b]);
    static_assert(TH_ % 4 == 0, "tile height must be a multiple of four");
    static_assert(NG == ND, "the vertical pass shares its row window between the two planes");
    constexpr int DH = DW / 2;                                   // half-quads per row
    for (int i = tid; i < (TH_ / 4) * DH; i += NTHR) {
        const int r = 4 * (i / DH), h = i % DH;
        const int x = tx0 + 2 * h;
        if (EDGE && (ty0 + r >= nr || x >= nc)) continue;
        float2 ox[4], oy[4];
        vgrad_2x4<NG, ND, DW, false>(D + (r + R - NG / 2) * DW + 2 * h, E + (r + R - ND / 2) * DW + 2 * h, kg, kd, ox, oy);
        const unsigned r_b0 = 3u * (tile_b0 + __umul24((unsigned)r, row_bytes) + (unsigned)(8 * h));   // byte offset of (ty0 + r, x) in the records
#pragma unroll
        for (int dr = 0; dr < 4; dr++) {
            const int y = ty0 + r + dr;
            if (EDGE && y >= nr) break;
            const unsigned ob = r_b0 + (unsigned)dr * 3u * row_bytes;
            const float2 im = *reinterpret_cast<const float2 *>(C + (r + dr + R) * BW + HB + 2 * h);
            store_records(recp, ob, im, ox[dr], oy[dr], !EDGE || x + 1 < nc);
        }
    }
    STAGE_MARK(5);
}

template <typename TIn, bool SMOOTH, int NS, int NG, int ND, int TH_, int NTHR = 256, bool HRED = false>
__global__ __launch_bounds__(NTHR, KLT_L0_WAVES) void smooth_grad_rb(SmoothGradArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[TileLds<SMOOTH, NS, NG, ND, TH_, HRED>::total];
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH_;
    const int nc = a.dim_c[b] ? a.dim_c[b] : a.ncols, nr = a.dim_r[b] ? a.dim_r[b] : a.nrows;
    if (tx0 >= nc || ty0 >= nr) return;              // entries smaller than the grid extent (mixed pyramid levels)
    // every output of the tile inside the frame (and, with the fused reduction, inside the H1 plane): block-uniform
    const bool inside = tx0 + TW <= nc && ty0 + TH_ <= nr && (!HRED || tx0 / 4 + TW / 4 <= a.h1_nc);
    if (inside) smooth_grad_rb_tile<TIn, SMOOTH, NS, NG, ND, TH_, NTHR, HRED, false>(a, lds, nc, nr);
    else smooth_grad_rb_tile<TIn, SMOOTH, NS, NG, ND, TH_, NTHR, HRED, true>(a, lds, nc, nr);
}

// ------------------------------------------------------------------------------------------------------
// Streaming level-0 kernel: the stages of smooth_grad_rb<TIn, true, NS, 7, 7, 32, 256, true>, but a workgroup walks a segment of
// `seg_h` rows of a TW-column strip in bands of SB output rows and computes every row of every stage once.  The tiled kernel computes
// its vertical halo again in every tile (42 / 38 / 38 rows of stages 1 / 2 / 3 for 32 output rows); here the last NS - 1 horizontally
// smoothed rows and the last 6 rows of the two gradient intermediates are carried to the next band, and the halo is paid once per
// segment.  Same expressions and operation order as the tiled kernel (both call the stage primitives above), same virtual coordinates
// (header of this file).
//
// Band with output rows [y, y + SB), cbase = y + 3 (frame row of C row 0):
//   A  raw rows (f32)           A row i  = frame row cbase + rs + i        SB rows x AW      (region 1)
//   B  H-smoothed               B row j  = frame row cbase - rs + j        SB + 2 rs rows    rows [0, 2 rs) carried (Bc)
//   C  smoothed image           C row i  = frame row cbase + i             SB rows x BW      (region 1, over A)
//   DE gradient intermediates   DE row k = frame row cbase - 6 + k         SB + 6 rows       rows [0, 6) carried
// A DE row holds the D row (derivative taps along x) in floats [0, TW) and the E row (Gaussian taps) in [TW, 2 TW).  B lives in the DE
// rows past the carried six (dead once stage 2 has run; its last 2 rs rows are saved to Bc first).  The prologue band of a segment
// (PRO) fills the carries: C rows [SB - 6, SB) = frame rows [s0 - 3, s0 + 3), no gradient output.
// The H1 plane is stored from the C rows of [s0, s0 + seg_h); the pixel records of [y, y + SB) from each steady band's stage 4, the image
// taken from C -- its first three rows from Cc, the interior columns of the last three C rows of the band before (two slots, by band
// parity: a band reads one and fills the other).
// Two geometries are built: TW x SB = 64 x 32 (KLT_OPT_L0_STREAM 1) and 128 x 16 (value 2).  Stages 0-2 run on the strip plus HB = 12 halo
// columns a side, (TW + 24) / TW of the output: 1.375 for 64 columns, 1.19 for 128.  A band is 2048 output pixels either way, and
// every carry scales with the strip width only; the wide strip's band is half as high so that the LDS still allows four workgroups per CU.
// (In the streaming templates TW is the template parameter; it hides the tiled kernels' file-level TW = 64.)
template <int NS, int TW, int SB>
struct StreamLds {
    static_assert(TW % 8 == 0 && SB % 4 == 0 && SB >= 6 + 2 * (NS / 2), "quads, 2 x 4 work items, prologue rows inside one band");
    static constexpr int HB = 12, rs = NS / 2;
    static constexpr int AW = TW + 2 * HB + 8, BW = TW + 2 * HB, DEW = 2 * TW;
    static constexpr int R1 = SB * AW;                           // A, then C
    static constexpr int NDE = (SB + 6) * DEW;                   // DE (B over its rows >= 6)
    static constexpr int NBC = 2 * rs * BW;                      // Bc
    static constexpr int NCC = 2 * 3 * TW;                       // Cc: two slots of three C rows' interior columns
    static constexpr int total = R1 + NDE + NBC + NCC;
    static_assert((SB + 2 * rs) * BW <= SB * DEW, "B must fit in the DE rows past the carried ones");
};

// Taps read from the kernel argument (the SmoothGradArgs at offset 0 of the kernarg segment) where they are used: the address goes through
// an empty asm statement so that the compiler cannot hoist the scalar loads out of the band loop (the four tap sets held across it spill)
// (smooth_grad_stream keeps its SmoothGradArgs as its first parameter for this.)
template <int NT>
__device__ __forceinline__ void load_taps_here(TapRegs<NT> &r, const size_t arg_offset)
{
    typedef const __attribute__((address_space(4))) char *kptr;
    kptr p = (kptr)__builtin_amdgcn_kernarg_segment_ptr() + arg_offset;
    asm volatile("" : "+s"(p));
#pragma unroll
    for (int i = 0; i < NT; i++) r.k[i] = ((const __attribute__((address_space(4))) double *)p)[i];
}

// u8 frames: the raw rows of a steady band (A rows [0, SB), 4 bytes per quad) are requested one band ahead and stay in flight in three
// registers (`pre`; 64 x 32: 768 quads, three per thread) while the band before runs its stages 1-4.  Edge bands read element by element through the reflect map (and wait for it).
// (128 x 16: 640 quads for 256 threads: the third register holds a quad of its own in half of the threads; the others repeat the last quad
// and do not store it.)
template <int TW, int SB>
constexpr int l0_stream_pre_regs() { return (SB * (TW + 32) / 4 + 255) / 256; }

// LEAN (KLT_OPT_L0_LAZY_GRAD): no gradients and no pixel records -- the gradient half of stage 3, stage 4, the DE rows, the Cc carry and
// their copies are left out, and the interior columns of the band's C rows go to the frame's compact image plane (a.cimg) instead, 16
// bytes per lane in coalesced rows.  Stages 0-2 and 3b, the halo, the prologue, the reflect map and the prefetch are the full kernel's;
// the LDS layout too (the DE rows past the carried six still hold B; the rest of that region and Cc lie unused).
template <typename TIn, int NS, int TW, int SB, bool ZC, bool EDGE, bool PRO, bool LEAN = false>
__device__ __forceinline__ void l0_stream_band(const SmoothGradArgs &a, float *const lds, const int nc, const int nr, const int tx0,
                                               const int cbase, const int s0, const int ylim, const int par, uint32_t (&pre)[l0_stream_pre_regs<TW, SB>()])
{
    constexpr bool PF = sizeof(TIn) == 1;                       // u8: raw rows fetched one band ahead
    constexpr int RQ = EDGE ? RAW_QUADS_NEVER : RAW_QUADS_ADDRESS_TESTED;   // (smooth_grad_stream has asked about the frame's address)
    STREAM_CLK_START;
    constexpr int NTHR = 256, NG = 7, ND = 7;
    using L = StreamLds<NS, TW, SB>;
    constexpr int HB = L::HB, rs = L::rs, AW = L::AW, BW = L::BW, DEW = L::DEW, DW = TW;
    constexpr int AQ = AW / 4, BQ = BW / 4, DQ = DW / 4;
    constexpr int CLO = PRO ? SB - 6 : 0;                        // C / DE rows made by this band: C [CLO, SB), DE [CLO + 6, SB + 6)
    constexpr int BLO = PRO ? CLO : 2 * rs;                      // B rows made: [BLO, SB + 2 rs)
    constexpr int ALO = BLO - 2 * rs;                            // A rows loaded: [ALO, SB)
    static_assert(ALO >= 0, "prologue rows");
    float *const A = lds, *const C = lds, *const DE = lds + L::R1, *const B = DE + 6 * DEW, *const Bc = DE + L::NDE;
    float *const Ccr = Bc + L::NBC + par * 3 * TW, *const Ccw = Bc + L::NBC + (par ^ 1) * 3 * TW;   // Cc slot read / filled by this band
    // tid goes through an empty asm statement once per band: the per-thread index math of the stages is then recomputed in each band
    // instead of being hoisted out of the band loop and held in registers across all stages
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int b = blockIdx.z;
    const TIn *__restrict__ raw = (const TIn *)a.raw[b];
    const unsigned row_bytes = 4u * (unsigned)nc;
    const unsigned band_b0 = (unsigned)cbase * row_bytes + 4u * (unsigned)tx0;   // byte offset of (cbase, tx0) in the f32 planes, mod 2^32
    constexpr int X0 = -(HB + 4);                                // frame column of A column 0, relative to the strip

    // ---- stage 0: raw rows -> registers; (after the previous band's stage 4) -> A, carried rows into place
    // (the host takes this kernel for frames of >= 2 strips and >= 64 rows: one reflection brings every index inside -- columns reach
    // TW + 15 past the last strip's first, rows SB + 1 + rs past the frame's last)
    {
        constexpr int NA = SB - ALO, N0 = NA * AQ, U0 = (N0 + NTHR - 1) / NTHR;
        typename RawQuad<TIn>::reg w[U0];
        if constexpr (PF && !PRO) {
            static_assert(U0 == sizeof(pre) / 4, "prefetched quads");
#pragma unroll
            for (int u = 0; u < U0; u++) w[u] = pre[u];
        } else {
            load_raw_block<TIn, NA, AQ, NTHR, RQ>(raw, nc, nr, cbase + rs + ALO, tx0 + X0, tid, w);
        }
        if (!PRO) __syncthreads();                               // the previous band's stage 4 has read DE
#pragma unroll
        for (int u = 0; u < U0; u++) {
            const int i = tid + u * NTHR;
            if (i < N0) *reinterpret_cast<float4 *>(A + ALO * AW + i * 4) = quad_f32(w[u]);
        }
        if (!PRO) {
            // B rows [0, 2 rs) from Bc; DE rows [SB, SB + 6) -> [0, 6)
            constexpr int NB = 2 * rs * BQ, NDQ = LEAN ? 0 : 6 * (DEW / 4);
            for (int i = NTHR - 1 - tid; i < NB + NDQ; i += NTHR) {
                if (i < NB) *reinterpret_cast<float4 *>(B + 4 * i) = *reinterpret_cast<const float4 *>(Bc + 4 * i);
                else *reinterpret_cast<float4 *>(DE + 4 * (i - NB)) = *reinterpret_cast<const float4 *>(DE + SB * DEW + 4 * (i - NB));
            }
        }
    }
    __syncthreads();
    STREAM_MARK(0);
    if constexpr (PF) {
        if (PRO || cbase - 3 + SB < ylim)                        // the A rows of the next steady band
            load_raw_block<uint8_t, SB, AQ, NTHR, RQ>(raw, nc, nr, (PRO ? s0 + 3 : cbase + SB) + rs, tx0 + X0, threadIdx.x, pre);
    }
    {
        TapRegs<NS> ks;
        load_taps_here(ks, offsetof(SmoothGradArgs, smooth.k));
        // ---- stage 1: horizontal smoothing, A -> B rows [BLO, SB + 2 rs)
        for (int i = tid; i < (SB + 2 * rs - BLO) * BQ; i += NTHR) {
            const int j = BLO + i / BQ, q = i % BQ;
            *reinterpret_cast<float4 *>(B + j * BW + 4 * q) = hsmooth_quad<NS>(A + (j - 2 * rs) * AW + 4 * q, ks);
        }
        __syncthreads();
        STREAM_MARK(1);
        // ---- stage 2: vertical smoothing, B -> C rows [CLO, SB)
        constexpr int BH = BW / 2, G2 = (SB - CLO + 3) / 4;
        for (int i = (tid + NTHR / 4) & (NTHR - 1); i < G2 * BH; i += NTHR) {
            const int r = CLO + 4 * (i / BH), h = i % BH;
            double v[2][NS + 3];
            widen_col_pair<NS + 3, BW>(B + r * BW + 2 * h, SB + 2 * rs - 1 - r, v);
#pragma unroll
            for (int dr = 0; dr < 4; dr++) {
                const int rr = r + dr;
                if (rr >= SB) break;
                *reinterpret_cast<float2 *>(C + rr * BW + 2 * h) = corr_pair<NS, 1>(v, dr, ks);
            }
        }
        // the last 2 rs rows of B are the next band's first ones
        for (int i = NTHR - 1 - tid; i < 2 * rs * BQ; i += NTHR)
            *reinterpret_cast<float4 *>(Bc + 4 * i) = *reinterpret_cast<const float4 *>(B + SB * BW + 4 * i);
    }
    __syncthreads();
    STREAM_MARK(2);
    if constexpr (LEAN) {
        // ---- stage 3 (lean): the interior columns of C rows [CLO, SB) that belong to the segment -> the compact image plane
        const plane_rsrc img = plane_of(a.cimg[b]);
        for (int i = (tid + NTHR / 2) & (NTHR - 1); i < (SB - CLO) * DQ; i += NTHR) {
            const int r = CLO + i / DQ, q = i % DQ;
            const int y = cbase + r, x = tx0 + 4 * q;
            if ((PRO && y < s0) || y >= ylim || (EDGE && x >= nc)) continue;
            const float4 v = *reinterpret_cast<const float4 *>(C + r * BW + HB + 4 * q);
            const unsigned ob = band_b0 + __umul24((unsigned)r, row_bytes) + 16u * (unsigned)q;      // byte offset of (y, x)
            if (!EDGE || x + 3 < nc) {
                plane_store4(img, ob, make_float2(v.x, v.y), make_float2(v.z, v.w));
            } else {
                plane_store(img, ob, v.x);
                if (x + 1 < nc) plane_store(img, ob + 4, v.y);
                if (x + 2 < nc) plane_store(img, ob + 8, v.z);
            }
        }
    } else {
        // ---- stage 3: horizontal pass of both gradients, C rows [CLO, SB) -> DE rows [CLO + 6, SB + 6)
        TapRegs<NG> kg;
        TapRegs<ND> kd;
        load_taps_here(kg, offsetof(SmoothGradArgs, ggauss.k));
        load_taps_here(kd, offsetof(SmoothGradArgs, gderiv.k));
        for (int i = (tid + NTHR / 2) & (NTHR - 1); i < (SB - CLO) * DQ; i += NTHR) {
            const int r = CLO + i / DQ, q = i % DQ;
            float4 d, e;
            hgrad_quad<NG, ND, ZC>(C + r * BW + 4 * q + (HB - 4), kg, kd, d, e);
            *reinterpret_cast<float4 *>(DE + (r + 6) * DEW + 4 * q) = d;
            *reinterpret_cast<float4 *>(DE + (r + 6) * DEW + DW + 4 * q) = e;
        }
        // the interior columns of C rows [SB - 3, SB): the first three image rows of the next band's stage 4
        for (int i = NTHR - 1 - tid; i < 3 * DQ; i += NTHR)
            *reinterpret_cast<float4 *>(Ccw + 4 * i) = *reinterpret_cast<const float4 *>(C + (SB - 3 + i / DQ) * BW + HB + 4 * (i % DQ));
    }
    {
        // ---- stage 3b: horizontal pass of the pyramid reduction at the columns 4x + 2 of the C rows of the segment (as in the tiled kernel)
        constexpr int NR = 21, HR = NR / 2;
        TapRegs<HR + 1> kr;
        load_taps_here(kr, offsetof(SmoothGradArgs, reduce.k));
        const plane_rsrc h1 = plane_of(a.h1[b]);
        const int h1_nc = a.h1_nc;
        const unsigned h1_row_bytes = 4u * (unsigned)h1_nc, h1_b0 = (unsigned)cbase * h1_row_bytes + (unsigned)tx0;   // (cbase, tx0 / 4)
        for (int i = tid; i < (SB - CLO) * (DQ / 2); i += NTHR) {
            const int r = CLO + i / (DQ / 2), xs = 2 * (i % (DQ / 2));
            const int y = cbase + r;
            float o[2];
            hreduce_pair<NR>(C + r * BW + 4 * xs + (HB - 8), kr, o);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int xg = tx0 / 4 + xs + k;
                if ((!PRO || y >= s0) && y < ylim && (!EDGE || xg < h1_nc))
                    plane_store(h1, h1_b0 + __umul24((unsigned)r, h1_row_bytes) + 4u * (unsigned)(xs + k), o[k]);
            }
        }
    }
    if (PRO || LEAN) {
        STREAM_MARK(3);                                          // (lean: the plane stores and stage 3b)
        return;
    }
    __syncthreads();
    STREAM_MARK(3);
    // ---- stage 4: vertical pass, output rows [cbase - 3, cbase - 3 + SB); the pixel records (image from C / Cc, gradx, grady) of two
    // adjacent pixels go out together: 24 contiguous bytes
    TapRegs<NG> kg;
    TapRegs<ND> kd;
    load_taps_here(kg, offsetof(SmoothGradArgs, ggauss.k));
    load_taps_here(kd, offsetof(SmoothGradArgs, gderiv.k));
    const plane_rsrc recp = plane_of(a.rec[b]);
    constexpr int DH = DW / 2;
    const int y0 = cbase - 3;
    const bool full = y0 + SB <= ylim;
    for (int i = tid; i < (SB / 4) * DH; i += NTHR) {
        const int r = 4 * (i / DH), h = i % DH;
        const int x = tx0 + 2 * h;
        if ((EDGE && x >= nc) || (!full && y0 + r >= ylim)) continue;
        float2 ox[4], oy[4];
        vgrad_2x4<NG, ND, DEW, ZC>(DE + r * DEW + 2 * h, DE + r * DEW + DW + 2 * h, kg, kd, ox, oy);
        const unsigned r_b0 = 3u * (band_b0 - 3u * row_bytes + __umul24((unsigned)r, row_bytes) + (unsigned)(8 * h));   // record of (y0 + r, x)
#pragma unroll
        for (int dr = 0; dr < 4; dr++) {
            if (!full && y0 + r + dr >= ylim) break;
            const int k = r + dr;                                // frame row y0 + k = C row k - 3
            const float *const im_row = k >= 3 ? C + (k - 3) * BW + HB : Ccr + k * TW;
            const float2 im = *reinterpret_cast<const float2 *>(im_row + 2 * h);
            store_records(recp, r_b0 + (unsigned)dr * 3u * row_bytes, im, ox[dr], oy[dr], !EDGE || x + 1 < nc);
        }
    }
    STREAM_MARK(4);
}

template <typename TIn, int NS, int TW, int SB, bool ZC, bool EDGE, bool LEAN>
__device__ __forceinline__ void l0_stream_segment(const SmoothGradArgs &a, float *const lds, const int nc, const int nr, const int tx0,
                                                  const int s0, const int ylim)
{
    uint32_t pre[l0_stream_pre_regs<TW, SB>()];
    l0_stream_band<TIn, NS, TW, SB, ZC, EDGE, true, LEAN>(a, lds, nc, nr, tx0, s0 + 3 - SB, s0, ylim, 1, pre);          // (fills Cc slot 0)
    for (int y = s0, par = 0; y < ylim; y += SB, par ^= 1) l0_stream_band<TIn, NS, TW, SB, ZC, EDGE, false, LEAN>(a, lds, nc, nr, tx0, y + 3, s0, ylim, par, pre);
}

// grid = (ceil(ncols / TW), ceil(nrows / seg_h), batch); seg_h a multiple of SB.
// `a` must stay the FIRST parameter: load_taps_here reads the taps at kernarg offset offsetof(SmoothGradArgs, ...).
template <typename TIn, int NS, bool ZC, int TW = 64, int SB = 32, bool LEAN = false>
__global__ __launch_bounds__(256, KLT_L0_WAVES) void smooth_grad_stream(SmoothGradArgs a, int seg_h)
{
    __shared__ __attribute__((aligned(16))) float lds[StreamLds<NS, TW, SB>::total];
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * TW, s0 = blockIdx.y * seg_h;
    const int nc = a.dim_c[b] ? a.dim_c[b] : a.ncols, nr = a.dim_r[b] ? a.dim_r[b] : a.nrows;
    if (tx0 >= nc || s0 >= nr) return;
    const int ylim = min(s0 + seg_h, nr);
    // A frame of a width divisible by 4 whose address is off its quads' alignment (an adopted frame starts at any byte: raw_quads_aligned,
    // l0_plan.h) takes the EDGE instantiation for every strip: that one never loads a quad.  For every other frame EDGE strips read
    // element by element as it is (h1_nc = nc / 4, so a strip is EDGE where tx0 + TW > 4 (nc / 4): its raw block, 16 columns wider a
    // side, leaves the frame or the width is no multiple of 4), and the other strips decide by the width alone, as they always have.
    // Asked here, once per workgroup, so that the band loop holds nothing for it.
    const bool off_quads = nc % 4 == 0 && !raw_quads_aligned(reinterpret_cast<uintptr_t>(a.raw[b]), nc, (int)sizeof(TIn));
    const bool inside = tx0 + TW <= nc && tx0 / 4 + TW / 4 <= a.h1_nc && !off_quads;
    STAGE_MARK(0);
    if (inside) l0_stream_segment<TIn, NS, TW, SB, ZC, false, LEAN>(a, lds, nc, nr, tx0, s0, ylim);
    else l0_stream_segment<TIn, NS, TW, SB, ZC, true, LEAN>(a, lds, nc, nr, tx0, s0, ylim);
    STAGE_MARK(5);
}

// ------------------------------------------------------------------------------------------------------
// Lean level-0 kernel, wave form (KLT_OPT_L0_LEAN_FORM): what smooth_grad_stream<..., LEAN> computes -- the smoothed image to the compact
// plane a.cimg and the horizontal pass of the first pyramid reduction to a.h1 -- with no workgroup barrier and no plane staged through
// LDS.  The lean banded kernel encloses 40 % of the full kernel's work in the full kernel's four barriers per band and runs at 0.64 of
// its VALU issue time (profiles/README.md); here a WAVEFRONT owns a strip and walks it down a segment of rows on its own.
//   Lane l owns the four columns x0 - 12 + 4 l ... + 3 of the strip at x0 = 232 * strip: lanes 3..60 are the strip's 232 output
//   columns, lanes 0-2 and 61-63 the 12-column halo of the 21-tap reduction.  Per row: the lane's raw quad (requested PD rows ahead,
//   held in registers), the samples left and right of it from the neighbouring lanes (a whole-wavefront DPP shift), the horizontal smoothing of the four
//   columns into a rotating window of the last NS H-smoothed rows in registers (the row loop is unrolled NS times, so the window's
//   indices are compile-time; kept widened for 5 taps, f32 and widened at use for 9), the vertical smoothing from the window, one
//   16-byte store to the compact plane, and the same quad into a padded row of LDS (LW_ROW) that only this wavefront touches, from which the lane
//   reads the rest of its 21-sample window (quads l - 2 .. l + 2 and the first sample of l + 3) for the H1 sample at column 4 l + 2 of
//   its quad.  One wavefront's LDS operations complete in order: s_waitcnt is all that orders the row's store and its loads.
// The NS - 1 rows above a segment are H-smoothed again (stage 1 only).  Rows go through the reflect map on the row index.  The first and
// the last strip of a frame, and frames whose width is no multiple of 4, read element by element through reflect_once and predicate
// their stores (EDGE).  Same virtual coordinates, expressions and operation order as the banded kernel (corr_quad, corr_regs and
// hreduce_pair's sum), so the same values (header of this file).  The host takes it for frames of >= 256 columns and >= NS rows: one
// reflection brings every index inside (columns reach 245 past the last strip's first, rows NS / 2 past either end).
constexpr int LW_COLS = 232, LW_HALO = 12, LW_WAVES = 4;         // output columns of a strip, halo columns a side, wavefronts per workgroup
// Wavefronts per SIMD the wave kernel asks the compiler for (its own constant: KLT_L0_WAVES bounds smooth_grad_rb and
// smooth_grad_stream).  All four instantiations fit 96 VGPRs without scratch under a bound of four and of five alike, so a SIMD holds five
// of them either way and the 9 x 34 x 16 = 4896 units of a sixteen-frame 1080p launch are resident at once (5120 slots;
// tests/test_l0_wave_regs.py holds the figure).  The bound itself stays four: the headline did not pass its gate with five
// (profiles/README.md).
#ifndef KLT_L0_WAVE_PER_SIMD
#define KLT_L0_WAVE_PER_SIMD 4
#endif
// A wavefront's LDS row: two quads of padding, the 64 quads of the lanes, two quads and one float of padding (kept a multiple of four
// floats).  Lane l reads quads l - 2 .. l + 2 and the first float of quad l + 3 at constant offsets from ONE per-lane address, without a
// clamp.  INVARIANT: nothing ever writes the padding, and only the six halo lanes (0 - 2, 61 - 63) can read it -- lanes 0 and 1 on the
// left, 61 - 63 on the right -- whose H1 sample is never stored (out_lane); an output lane's window 4 l - 8 .. 4 l + 12 lies inside
// quads 1 .. 63.  Whatever an earlier workgroup left in the padding therefore reaches no result.
constexpr int LW_PAD_L = 8, LW_PAD_R = 12, LW_ROW = LW_PAD_L + 256 + LW_PAD_R;
static_assert(LW_PAD_L >= 8 && LW_PAD_R >= 9 && LW_ROW % 4 == 0, "padding of the H1 window's reads");

// The raw samples of one row and lane in flight: the RawQuad register of the aligned path, four zero-extended bytes of a u8 edge strip
template <typename TIn, bool EDGE> struct WaveRaw { typedef typename RawQuad<TIn>::reg reg; };
template <> struct WaveRaw<uint8_t, true> { typedef uint4 reg; };
__device__ __forceinline__ uint32_t wave_quad(uint4 e) { return e.x | e.y << 8 | e.z << 16 | e.w << 24; }
__device__ __forceinline__ uint32_t wave_quad(uint32_t w) { return w; }
__device__ __forceinline__ float4 wave_quad(float4 v) { return v; }

// The value of lane l - 1 (UP = false) or l + 1 (UP = true) of the wavefront: a whole-wavefront DPP shift, which needs no index register
// and no LDS queue slot (ds_bpermute needs both).  Lane 0 has no lane below it and lane 63 none above: they get 0 (bound_ctrl), in samples
// that only reach columns of halo lanes which no stored output reads (lean_wave_segment).
template <bool UP> __device__ __forceinline__ uint32_t lane_next(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, UP ? 0x130 /* wave_shl:1 */ : 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
}
template <bool UP> __device__ __forceinline__ float lane_next(float v) { return __builtin_bit_cast(float, lane_next<UP>(__builtin_bit_cast(uint32_t, v))); }

template <typename TIn, int NS, bool EDGE>
__device__ __forceinline__ void lean_wave_segment(const SmoothGradArgs &a, float *const wrow /* 2 x LW_ROW floats of this wavefront */, const int b,
                                                  const int nc, const int nr, const int x0, const int s0, const int ylim)
{
    constexpr int rs = NS / 2, PD = NS % 3 == 0 ? 3 : NS;        // rows in flight: a divisor of the unroll count
    constexpr int NR = 21, HR = NR / 2;
    constexpr bool U8 = sizeof(TIn) == 1, NXT = rs > 3;          // (NXT: lane 63's first output reads one sample past its quad)
    typedef typename WaveRaw<TIn, EDGE>::reg raw_t;
    typedef typename std::conditional<(NS <= 5), double, float>::type win_t;
    typedef volatile __attribute__((address_space(3))) f32x4 *lds_quad_ptr;
    typedef const volatile __attribute__((address_space(3))) float *lds_f32_ptr;
    const int lane = threadIdx.x & 63;
    const int cx = x0 - LW_HALO + 4 * lane;                      // the lane's first column (virtual)
    const bool out_lane = lane >= LW_HALO / 4 && lane < 64 - LW_HALO / 4;
    const plane_rsrc rawp = plane_of(a.raw[b]), img = plane_of(a.cimg[b]), h1 = plane_of(a.h1[b]);
    const int h1_nc = a.h1_nc;
    const unsigned raw_row_b = (unsigned)nc * (unsigned)sizeof(TIn);
    // byte offsets of the lane's columns in a raw row: the quad's (aligned path) or each element's through the reflect map; `xn`: the
    // sample right of lane 63's quad
    unsigned xo[EDGE ? 4 : 1];
    if constexpr (EDGE) {
#pragma unroll
        for (int k = 0; k < 4; k++) xo[k] = (unsigned)reflect_once(cx + k, nc) * (unsigned)sizeof(TIn);
    } else {
        xo[0] = (unsigned)cx * (unsigned)sizeof(TIn);
    }
    const unsigned xn = (unsigned)(EDGE ? reflect_once(cx + 4, nc) : cx + 4) * (unsigned)sizeof(TIn);
    // LDS: the lane's address in a padded row is that of quad l - 2; its own quad is two quads on (layout and invariant: LW_ROW above)
    float *const wlane = wrow + 4 * lane;
    const int T = ylim - s0 + 2 * rs;                            // H-smoothed rows of the segment: step t makes frame row s0 - rs + t

    auto request = [&](int t, raw_t &q, float &nx) {
        const unsigned row_b = (unsigned)reflect_once(s0 - rs + t, nr) * raw_row_b;
        if constexpr (!EDGE) {
            if constexpr (U8) q = __builtin_amdgcn_raw_buffer_load_b32(rawp, row_b + xo[0], 0, 0);
            else q = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rawp, row_b + xo[0], 0, 0));
        } else if constexpr (U8) {
            q.x = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rawp, row_b + xo[0], 0, 0); q.y = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rawp, row_b + xo[1], 0, 0);
            q.z = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rawp, row_b + xo[2], 0, 0); q.w = (uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rawp, row_b + xo[3], 0, 0);
        } else {
            q.x = plane_load(rawp, row_b + xo[0]); q.y = plane_load(rawp, row_b + xo[1]);
            q.z = plane_load(rawp, row_b + xo[2]); q.w = plane_load(rawp, row_b + xo[3]);
        }
        if constexpr (NXT) {
            if (lane == 63) {
                if constexpr (U8) nx = (float)(uint8_t)__builtin_amdgcn_raw_buffer_load_b8(rawp, row_b + xn, 0, 0);
                else nx = plane_load(rawp, row_b + xn);
            }
        }
    };

    TapRegs<NS> ks;
    TapRegs<HR + 1> kr;
    load_taps(ks, a.smooth);
    load_taps(kr, a.reduce);
    raw_t pre[PD];
    float nxt[PD] = {};
#pragma unroll
    for (int u = 0; u < PD; u++)
        if (u < T) request(u, pre[u], nxt[u]);
    win_t win[NS][4];
    for (int t0 = 0; t0 < T; t0 += NS) {
#pragma unroll
        for (int u = 0; u < NS; u++) {
            const int t = t0 + u;
            if (t >= T) break;
            // ---- the row's raw samples: the lane's quad, and the quads of its neighbours
            const typename RawQuad<TIn>::reg w = wave_quad(pre[u % PD]);
            const float nx = nxt[u % PD];
            if (t + PD < T) request(t + PD, pre[u % PD], nxt[u % PD]);
            float4 mid = quad_f32(w), lo, hi;
            if constexpr (U8) {
                lo = unpack_u8x4(lane_next<false>(w));
                hi = unpack_u8x4(lane_next<true>(w));
            } else {
                lo.x = rs > 3 ? lane_next<false>(mid.x) : 0.f; lo.y = rs > 2 ? lane_next<false>(mid.y) : 0.f;
                lo.z = rs > 1 ? lane_next<false>(mid.z) : 0.f; lo.w = lane_next<false>(mid.w);
                hi.x = lane_next<true>(mid.x); hi.y = rs > 1 ? lane_next<true>(mid.y) : 0.f;
                hi.z = rs > 2 ? lane_next<true>(mid.z) : 0.f; hi.w = rs > 3 ? lane_next<true>(mid.w) : 0.f;
            }
            if constexpr (NXT) if (lane == 63) hi.x = nx;
            // ---- horizontal smoothing of the four columns -> the window's slot u
            {
                double v[12];
                v[0] = (double)lo.x; v[1] = (double)lo.y; v[2] = (double)lo.z; v[3] = (double)lo.w;
                v[4] = (double)mid.x; v[5] = (double)mid.y; v[6] = (double)mid.z; v[7] = (double)mid.w;
                v[8] = (double)hi.x; v[9] = (double)hi.y; v[10] = (double)hi.z; v[11] = (double)hi.w;
                const float4 hq = corr_quad<NS, 1>(v, ks);
                win[u][0] = (win_t)hq.x; win[u][1] = (win_t)hq.y; win[u][2] = (win_t)hq.z; win[u][3] = (win_t)hq.w;
            }
            if (t < 2 * rs) continue;
            // ---- vertical smoothing: frame row y from the window (the row rs + j below y's first sits in slot (u + 1 + j) mod NS)
            const int y = s0 + t - 2 * rs;
            float c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                double v[NS];
#pragma unroll
                for (int j = 0; j < NS; j++) v[j] = (double)win[(u + 1 + j) % NS][k];
                c[k] = corr_regs<NS, 1>(v + rs, ks);
            }
            if (out_lane) {
                const unsigned ob = 4u * ((unsigned)y * (unsigned)nc + (unsigned)cx);
                if (!EDGE || cx + 3 < nc) {
                    plane_store4(img, ob, make_float2(c[0], c[1]), make_float2(c[2], c[3]));
                } else {
                    if (cx < nc) plane_store(img, ob, c[0]);
                    if (cx + 1 < nc) plane_store(img, ob + 4, c[1]);
                    if (cx + 2 < nc) plane_store(img, ob + 8, c[2]);
                }
            }
            // ---- the H1 sample at column cx + 2: the row through this wavefront's LDS slot (by row parity), then the 21-tap sum
            float *const slot = wlane + (t & 1) * LW_ROW;        // (quad l - 2 of the row's slot)
            f32x4 cq;
            cq.x = c[0]; cq.y = c[1]; cq.z = c[2]; cq.w = c[3];
            *(lds_quad_ptr)(slot + 8) = cq;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // hreduce_pair's sum at the centre m[HR] of the window m[0 .. 20] = quads l - 2, l - 1, c, l + 1, l + 2 and the first sample of
            // l + 3: the samples are read and widened in the order the sum takes them, the centre, then (m[0], m[20]) ... (m[9], m[11]),
            // in three stages so that a third of the window is live at a time (same operations, same order, same roundings; the LDS reads are
            // volatile and keep their order, and the scheduler leaves the widenings with their stage: no scheduling barrier is needed)
            auto pair = [&](double acc, float lo_s, float hi_s, int j) { return acc + ((double)lo_s + (double)hi_s) * kr.k[j]; };
            double acc = (double)c[2] * kr.k[HR];
            {
                const f32x4 qa = *(lds_quad_ptr)(slot), qe = *(lds_quad_ptr)(slot + 16);
                const float qf = *(lds_f32_ptr)(slot + 20);
                acc = pair(acc, qa.x, qf, 0);
                acc = pair(acc, qa.y, qe.w, 1);
                acc = pair(acc, qa.z, qe.z, 2);
                acc = pair(acc, qa.w, qe.y, 3);
                const f32x4 qb = *(lds_quad_ptr)(slot + 4), qd = *(lds_quad_ptr)(slot + 12);
                acc = pair(acc, qb.x, qe.x, 4);
                acc = pair(acc, qb.y, qd.w, 5);
                acc = pair(acc, qb.z, qd.z, 6);
                acc = pair(acc, qb.w, qd.y, 7);
                acc = pair(acc, c[0], qd.x, 8);
                acc = pair(acc, c[1], c[3], 9);
            }
            const int xg = cx / 4;
            if (out_lane && (!EDGE || xg < h1_nc)) plane_store(h1, 4u * ((unsigned)y * (unsigned)h1_nc + (unsigned)xg), (float)acc);
        }
    }
}

// grid = ceil(units / 4) workgroups of four wavefronts; unit = (frame * nsegs + segment) * nstrips + strip, any four units to a workgroup
// (a wavefront per SIMD).  `a` stays the first parameter, as for smooth_grad_stream.
template <typename TIn, int NS>
__global__ __launch_bounds__(64 * LW_WAVES, KLT_L0_WAVE_PER_SIMD) void smooth_grad_lean_wave(SmoothGradArgs a, int seg_h, int nstrips, int nsegs, int nunits)
{
    __shared__ __attribute__((aligned(16))) float lds[LW_WAVES * 2 * LW_ROW];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.x * LW_WAVES + wave;
    if (unit >= nunits) return;
    const int strip = unit % nstrips, rest = unit / nstrips, seg = rest % nsegs, b = rest / nsegs;
    const int nc = a.dim_c[b] ? a.dim_c[b] : a.ncols, nr = a.dim_r[b] ? a.dim_r[b] : a.nrows;
    const int x0 = strip * LW_COLS, s0 = seg * seg_h;
    if (x0 >= nc || s0 >= nr) return;
    const int ylim = min(s0 + seg_h, nr);
    // every column the strip reads inside the frame, its quads aligned (by this frame's own address: wavefront-uniform)
    const bool inside = raw_quads_aligned(reinterpret_cast<uintptr_t>(a.raw[b]), nc, (int)sizeof(TIn)) && x0 >= LW_HALO && x0 + LW_COLS + LW_HALO + (NS / 2 > 3 ? 4 : 0) <= nc && x0 / 4 + LW_COLS / 4 <= a.h1_nc;
    if (inside) lean_wave_segment<TIn, NS, false>(a, lds + wave * (2 * LW_ROW), b, nc, nr, x0, s0, ylim);
    else lean_wave_segment<TIn, NS, true>(a, lds + wave * (2 * LW_ROW), b, nc, nr, x0, s0, ylim);
}

// The f32-rounded horizontal result is kept in LDS as the double it widens to (one widening per sample instead of one
// per tap of the vertical pass); the source tile stays f32 (an f64 tile was measured slower: half the LDS matters more).
template <int NT, int STRIDE>
__device__ __forceinline__ float correlate_sym_f64(const double *c, const TapRegs<NT> &t)
{
    constexpr int H = NT / 2;
    double acc = c[0] * t.k[H];
#pragma unroll
    for (int jj = -H; jj < 0; jj++) acc = acc + (c[jj * STRIDE] + c[-jj * STRIDE]) * t.k[H + jj];
    return (float)acc;
}

// TS = element type of the source tile in LDS: double (widened once at load) or float (half the LDS, widened per tap)
template <int SS, int NT, int NTHR, typename TS, int OW = ::OW_DEFAULT, int OH = ::OH_DEFAULT>
__global__ __launch_bounds__(NTHR) void pyr_reduce_fast(PyrReduceArgs a)
{
    constexpr int r = NT / 2;
    constexpr int SW = (OW - 1) * SS + 2 * r + 1, SH = (OH - 1) * SS + 2 * r + 1;
    constexpr int PW = (SW + SS - 1) / SS, ROWLEN = PW * SS;
    extern __shared__ __attribute__((aligned(16))) double dlds[];
    double *const Hd = dlds;                                     // [SH][OW]
    TS *const S = reinterpret_cast<TS *>(dlds + SH * OW);        // [SH][SS planes][PW]
    const int tid = threadIdx.x, b = blockIdx.z;
    const int xs0 = blockIdx.x * OW, ys0 = blockIdx.y * OH;
    const int gx0 = xs0 * SS + SS / 2 - r, gy0 = ys0 * SS + SS / 2 - r;
    const float *__restrict__ src = a.src[b];
    const int nc = a.src_nc, nr = a.src_nr;
    TapRegs<NT> k;
    load_taps(k, a.taps);
    STAGE_MARK(0);

    // tile load: one aligned 16-byte quad per step where the row allows it (gx0 is a multiple of 4 columns)
    constexpr int SQ = (SW + 3) / 4;
    const bool quads = (nc & 3) == 0;
    // tiles inside the frame: all quads of the thread are requested before the first is used (the general loop waits for
    // each load in turn, and the tile load is 2.3 of the 3.7 us a workgroup lives)
    constexpr int NQ = SH * SQ, QPT = (NQ + NTHR - 1) / NTHR;
    const bool interior = quads && (gx0 & 3) == 0 && gx0 >= 0 && gy0 >= 0 && gx0 + 4 * SQ <= nc && gy0 + SH <= nr;
    if (interior) {
        const plane_rsrc srcp = plane_of(src);                           // raw buffer loads: 32-bit byte offsets
        const unsigned src_b0 = 4u * ((unsigned)gy0 * (unsigned)nc + (unsigned)gx0);
        float4 v[QPT];
#pragma unroll
        for (int u = 0; u < QPT; u++) {
            const int i = min(tid + u * NTHR, NQ - 1);                    // clamped: the last threads repeat the last quad
            const int rr = i / SQ, q = i - rr * SQ;
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(srcp, src_b0 + 4u * (__umul24((unsigned)rr, (unsigned)nc) + 4u * (unsigned)q), 0, 0);
            v[u] = __builtin_bit_cast(float4, w);
        }
#pragma unroll
        for (int u = 0; u < QPT; u++) {
            const int i = tid + u * NTHR;
            if (i < NQ) {
                const int rr = i / SQ, q = i - rr * SQ;
                TS *dst = S + rr * ROWLEN;
                const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    const int c = 4 * q + w;
                    if (c < SW) dst[(c % SS) * PW + c / SS] = (TS)e[w];
                }
            }
        }
    } else if (nc >= 2 * SW && nr >= 2 * SH) {
        // frame-edge tiles of frames large enough that one reflection brings every index inside: branch-free index map,
        // every element load of the thread in flight together
        constexpr int NE = SH * SW, EPT = (NE + NTHR - 1) / NTHR;
        float e[EPT];
#pragma unroll
        for (int u = 0; u < EPT; u++) {
            const int i = min(tid + u * NTHR, NE - 1);
            const int y = gy0 + i / SW, x = gx0 + i % SW;
            e[u] = src[(size_t)reflect_once(y, nr) * nc + reflect_once(x, nc)];
        }
#pragma unroll
        for (int u = 0; u < EPT; u++) {
            const int i = tid + u * NTHR;
            const int rr = i / SW, c = i % SW;
            if (i < NE) S[rr * ROWLEN + (c % SS) * PW + c / SS] = (TS)e[u];
        }
    } else
    for (int i = tid; i < SH * SQ; i += NTHR) {
        const int rr = i / SQ, q = i % SQ;
        const int gy = reflect_fast(gy0 + rr, nr);
        const float *row = src + (size_t)gy * nc;
        const int x = gx0 + 4 * q;
        TS *dst = S + rr * ROWLEN;
        if (quads && x >= 0 && x + 3 < nc && 4 * q + 3 < SW) {
            const float4 v = *reinterpret_cast<const float4 *>(row + x);
            dst[((4 * q) % SS) * PW + (4 * q) / SS] = (TS)v.x;
            dst[((4 * q + 1) % SS) * PW + (4 * q + 1) / SS] = (TS)v.y;
            dst[((4 * q + 2) % SS) * PW + (4 * q + 2) / SS] = (TS)v.z;
            dst[((4 * q + 3) % SS) * PW + (4 * q + 3) / SS] = (TS)v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int c = 4 * q + e;
                if (c < SW) dst[(c % SS) * PW + c / SS] = (TS)row[reflect_fast(gx0 + c, nc)];
            }
        }
    }
    __syncthreads();
    STAGE_MARK(1);
    for (int i = tid; i < SH * OW; i += NTHR) {
        const int rr = i / OW, xs = i % OW;
        const TS *row = S + rr * ROWLEN + xs;            // column xs*SS + r + j lives at plane (r+j)%SS, index xs + (r+j)/SS
        double acc = (double)row[(r % SS) * PW + r / SS] * k.k[r];
#pragma unroll
        for (int jj = -r; jj < 0; jj++) {
            const double lo = (double)row[((r + jj) % SS) * PW + (r + jj) / SS];
            const double hi = (double)row[((r - jj) % SS) * PW + (r - jj) / SS];
            acc = acc + (lo + hi) * k.k[r + jj];
        }
        Hd[i] = (double)(float)acc;                      // the f32 rounding between the passes
    }
    __syncthreads();
    STAGE_MARK(2);
    if (tid < OW * OH) {
        const int xs = tid % OW, ys = tid / OW;
        const int ox = xs0 + xs, oy = ys0 + ys;
        if (ox < a.dst_nc && oy < a.dst_nr)
            a.dst[b][(size_t)oy * a.dst_nc + ox] = correlate_sym_f64<NT, OW>(Hd + (ys * SS + r) * OW + xs, k);
    }
    STAGE_MARK(5);
}

template <int SS, int NT, typename TS, int OW, int OH>
constexpr size_t pyr_reduce_fast_lds()
{
    constexpr int r = NT / 2;
    constexpr int SW = (OW - 1) * SS + 2 * r + 1, SH = (OH - 1) * SS + 2 * r + 1;
    constexpr int PW = (SW + SS - 1) / SS;
    return sizeof(double) * (size_t)(SH * OW) + sizeof(TS) * (size_t)(SH * PW * SS);
}

template <int SS, int NT, int NTHR, typename TS, int OW, int OH>
static int launch_pyr_reduce_fast(hipStream_t s, const PyrReduceArgs &a, int batch)
{
    constexpr size_t l = pyr_reduce_fast_lds<SS, NT, TS, OW, OH>();
    if (int e = set_lds(pyr_reduce_fast<SS, NT, NTHR, TS, OW, OH>, l)) return e;
    const dim3 grid((a.dst_nc + OW - 1) / OW, (a.dst_nr + OH - 1) / OH, batch);
    klt_launch((pyr_reduce_fast<SS, NT, NTHR, TS, OW, OH>), grid, dim3(NTHR), (unsigned)l, s, a);
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// Second half of the fused first reduction: level 1 (ys, xs) = V(H1)(4 ys + 2, xs), H1 = the horizontally reduced level-0 image
// written by smooth_grad_rb<..., HRED>.  Tile = 64 columns x 16 output rows; a thread makes 4 consecutive output rows of one
// column from 33 input rows (widened once).  Rows beyond the frame are read through the reflect map, as the reference does.
template <int SS, int NT>
__global__ __launch_bounds__(256) void pyr_vreduce_kernel(PyrReduceArgs a)
{
    constexpr int r = NT / 2, VW = 64, VH = 16, SH = (VH - 1) * SS + 2 * r + 1;       // 81 source rows
    __shared__ float T[SH * VW];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int xs0 = blockIdx.x * VW, ys0 = blockIdx.y * VH;
    const int nc = a.dst_nc, nr = a.src_nr;                     // H1 is src_nr rows x dst_nc columns
    const plane_rsrc src = plane_of(a.src[b]);                  // raw buffer loads: 32-bit byte offsets, no 64-bit multiply-add per row
    TapRegs<r + 1> k;
#pragma unroll
    for (int t = 0; t <= r; t++) k.k[t] = a.taps.k[t];
    const int gy0 = ys0 * SS + SS / 2 - r;
    {
        constexpr int N = SH * VW, U = (N + 255) / 256;
        const int col = min(xs0 + (tid & 63), nc - 1);
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {                            // clamped, unconditional; all loads in flight together
            const int rr = min((tid >> 6) + 4 * u, SH - 1);
            const int y = min(max(reflect_once(gy0 + rr, nr), 0), nr - 1);   // (frames shorter than the halo never take this kernel)
            v[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src, 4u * (__umul24((unsigned)y, (unsigned)nc) + (unsigned)col), 0, 0));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int rr = (tid >> 6) + 4 * u;
            if (rr < SH) T[rr * VW + (tid & 63)] = v[u];
        }
    }
    __syncthreads();
    const int xs = tid & 63, yq = tid >> 6;                      // output rows ys0 + 4 yq .. + 3
    const plane_rsrc dst = plane_of(a.dst[b]);
    double v[3 * SS + 2 * r + 1];                                // 33 rows
#pragma unroll
    for (int j = 0; j < 3 * SS + 2 * r + 1; j++) v[j] = (double)T[(4 * yq * SS + j) * VW + xs];
#pragma unroll
    for (int o = 0; o < 4; o++) {
        const double *c = v + o * SS + r;
        double acc = c[0] * k.k[r];
#pragma unroll
        for (int jj = -r; jj < 0; jj++) acc = acc + (c[jj] + c[-jj]) * k.k[r + jj];
        const int oy = ys0 + 4 * yq + o, ox = xs0 + xs;
        if (oy < a.dst_nr && ox < a.dst_nc) plane_store(dst, 4u * (__umul24((unsigned)oy, (unsigned)a.dst_nc) + (unsigned)ox), (float)acc);
    }
}

// (A one-launch-per-level kernel -- vertical reduction from the previous level's H planes, the level's gradients and the next
// level's H planes in one workgroup -- existed in round 1 as KLT_OPT_FUSED_LEVELS: bit-identical, 12 us per level against 5 + 5 + 5
// for the three small launches, because its phases are serial and latency-bound inside a workgroup.  Removed in round 2.)
// (The last level's reduction inside the merged gradient launch -- 1024-thread workgroups, a 32x8 tile + halo of 3 reduced into LDS, halo
// positions beyond the frame reflected there, gradient passes on it; the gradients of the levels in between as further workgroups of
// the same launch -- was built and measured in round 2 as well: bit-identical (all parity tests), 10.5 us per launch against 4.9 + 5.3 for
// the two launches it replaces, 0.0567 vs 0.0557 ms per pair on one stream.  The launch boundary it saves (1.5-2 us) is less than
// what the longer serial chain of a workgroup costs; not kept.)

}  // namespace

static_assert(TW == L0_TILE_W && TH == L0_TILE_H && LW_COLS == L0_WAVE_COLS && LW_WAVES == L0_WAVE_WAVES, "l0_plan.h plans grids for these tiles");

size_t pyr_reduce_lds_bytes(int ss, int ntaps)
{
    const int r = ntaps / 2;
    const int SW = (OW - 1) * ss + 2 * r + 1, SH = (OH - 1) * ss + 2 * r + 1;
    const int PW = (SW + ss - 1) / ss;
    return sizeof(float) * (size_t)(SH * PW * ss + SH * OW);
}

template <typename K>
static int set_lds(K kernel, size_t lds)
{
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

int launch_pyr_vreduce(hipStream_t s, const PyrReduceArgs &a, int batch)
{
    const dim3 grid((a.dst_nc + 63) / 64, (a.dst_nr + 15) / 16, batch);
    klt_launch((pyr_vreduce_kernel<4, 21>), grid, dim3(256), 0, s, a);
    return 0;
}

// The banded streaming kernels of one input type, smoothing tap count and geometry
template <typename TIn, int NS, int STRIP, int BAND>
static void launch_smooth_grad_banded(hipStream_t s, const SmoothGradArgs &a, const L0Plan &p, const dim3 &g, const dim3 &blk)
{
    if (p.lean) { klt_launch((smooth_grad_stream<TIn, NS, false, STRIP, BAND, true>), g, blk, 0, s, a, p.seg); return; }
    if constexpr (sizeof(TIn) == 1) if (p.zc) { klt_launch((smooth_grad_stream<TIn, NS, true, STRIP, BAND>), g, blk, 0, s, a, p.seg); return; }
    klt_launch((smooth_grad_stream<TIn, NS, false, STRIP, BAND>), g, blk, 0, s, a, p.seg);
}

// The register-blocked and streaming kernels of one input type and smoothing tap count (SMOOTH = false: gradients only, NS = 1)
// (28- / 24- / 20-row tiles -- 32.0 / 28.4 / 24.8 KB of LDS, five / five / six workgroups per CU -- were measured in
// round 2: 29.9 / 29.9 / 30.4 us event-timed against 28.1 for the 32-row tile: the extra halo work outweighs the occupancy)
// (three / two workgroups per CU instead of four -- dynamic LDS padding, same kernel -- read 0.0379 / 0.0382 ms per pair with
// three pairs in flight against 0.0365, and 0.0576 against 0.0556 on one stream: round 2)
template <typename TIn, bool SMOOTH, int NS>
static void launch_smooth_grad_rb(hipStream_t s, const SmoothGradArgs &a, const L0Plan &p)
{
    const dim3 g(p.gx, p.gy, p.gz), blk(p.block);
    if constexpr (SMOOTH) if (p.hred) {
        if (p.family == L0_FAMILY_WAVE) klt_launch((smooth_grad_lean_wave<TIn, NS>), g, blk, 0, s, a, p.seg, p.nstrips, p.nsegs, p.units);
        else if (p.family == L0_FAMILY_BANDED && p.strip == L0W_TW) launch_smooth_grad_banded<TIn, NS, L0W_TW, L0W_SB>(s, a, p, g, blk);
        else if (p.family == L0_FAMILY_BANDED) launch_smooth_grad_banded<TIn, NS, L0S_TW, L0S_SB>(s, a, p, g, blk);
        else klt_launch((smooth_grad_rb<TIn, true, NS, 7, 7, 32, 256, true>), g, blk, 0, s, a);
        return;
    }
    if (p.tile_rows == 32) klt_launch((smooth_grad_rb<TIn, SMOOTH, NS, 7, 7, 32>), g, blk, 0, s, a);
    else klt_launch((smooth_grad_rb<TIn, SMOOTH, NS, 7, 7, 16>), g, blk, 0, s, a);
}

// Executes a plan (plan_level0, l0_plan.h): selects the instantiation by input type, smoothing tap count and the plan's form, decides nothing
int launch_smooth_grad(hipStream_t s, const SmoothGradArgs &a, const L0Plan &p)
{
    const int kind = p.kind;
    if (p.family != L0_FAMILY_TILED_LDS) {
        const int ns = kind < 2 ? a.smooth.n : 1;
        if (kind == 0 && ns == 5) launch_smooth_grad_rb<uint8_t, true, 5>(s, a, p);
        if (kind == 1 && ns == 5) launch_smooth_grad_rb<float, true, 5>(s, a, p);
        if (kind == 0 && ns == 9) launch_smooth_grad_rb<uint8_t, true, 9>(s, a, p);
        if (kind == 1 && ns == 9) launch_smooth_grad_rb<float, true, 9>(s, a, p);
        if (kind == 2) launch_smooth_grad_rb<float, false, 1>(s, a, p);
        if (kind == 3) launch_smooth_grad_rb<uint8_t, false, 1>(s, a, p);
        return 0;
    }
    const dim3 grid(p.gx, p.gy, p.gz), block(p.block);
    int e = 0;
    switch (kind) {
    case 0: if ((e = set_lds(smooth_grad_kernel<uint8_t, true>, p.lds))) return e;
            klt_launch((smooth_grad_kernel<uint8_t, true>), grid, block, p.lds, s, a); break;
    case 1: if ((e = set_lds(smooth_grad_kernel<float, true>, p.lds))) return e;
            klt_launch((smooth_grad_kernel<float, true>), grid, block, p.lds, s, a); break;
    case 2: if ((e = set_lds(smooth_grad_kernel<float, false>, p.lds))) return e;
            klt_launch((smooth_grad_kernel<float, false>), grid, block, p.lds, s, a); break;
    default: if ((e = set_lds(smooth_grad_kernel<uint8_t, false>, p.lds))) return e;
            klt_launch((smooth_grad_kernel<uint8_t, false>), grid, block, p.lds, s, a); break;
    }
    return 0;
}

int launch_pyr_reduce(hipStream_t s, const PyrReduceArgs &a, int batch)
{
    const dim3 grid((a.dst_nc + OW - 1) / OW, (a.dst_nr + OH - 1) / OH, batch), block(256);
    if (a.taps.sym == 1) {
        // measured at cfg-2 (us per launch, two frames, both levels averaged): f32 tile / 1024 threads 11.6,
        // f64 tile / 1024 threads 12.4, f32 / 512 14.1, f64 / 512 15.4 (profiles/README.md)
        // tile shapes 64x8, 32x16, 32x4 and 16x16 were measured too: 32x8 is the fastest (profiles/README.md)
        if (a.ss == 4 && a.taps.n == 21) return launch_pyr_reduce_fast<4, 21, 1024, float, 32, 8>(s, a, batch);
        if (a.ss == 2 && a.taps.n == 11) return launch_pyr_reduce_fast<2, 11, 512, float, 32, 8>(s, a, batch);
    }
    const size_t lds = pyr_reduce_lds_bytes(a.ss, a.taps.n);
    if (int e = set_lds(pyr_reduce_kernel, lds)) return e;
    hipLaunchKernelGGL(pyr_reduce_kernel, grid, block, lds, s, a);
    return 0;
}
