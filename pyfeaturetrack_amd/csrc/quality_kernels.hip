// Per-feature track quality (gfx950): klt_track_quality_async.  One launch reads two feature lists and level 0 of two frames and writes one
// 16-byte klt_quality record per feature -- the residue that tc.max_residue tests, a normalised cross-correlation that a brightness change
// leaves alone, and the smaller eigenvalue of the gradient matrix under the window at the new position.  It decides nothing: thresholds
// are the caller's (DESIGN.md section 9f has the rule once more, with its reasons).
//
// THE RULE, per feature i, with in / out record i of the two lists, w the window, n = w * w, hw = w / 2, k row-major over the window.
//   measured   in.val >= 0 and out.val == KLT_TRACKED (a slot refilled by a replacement pass, val > 0, is not measured); both positions
//              inside the frame, 0 <= x < ncols and 0 <= y < nrows, written so that NaN and infinities fail and tested BEFORE any
//              conversion to int; both windows pass the sampler's own test ix-hw >= 0, iy-hw >= 0, ix+hw+2 <= ncols, iy+hw+2 <= nrows
//              with ix = (int)x.  Every other record is (0, 0, 0, val = 0); a measured one has val = 1.
//   samples    T_k of frame 1's level-0 image at (in.x, in.y); S_k, Sgx_k, Sgy_k of frame 2's image and gradients at (out.x, out.y): the
//              tracker's bilinear expression (make_bilinear / sample).
//   residue    the f32 |T_k - S_k| added with numpy's pairwise f32 sum, one IEEE f32 division by (float)n: trackFeatures.py:124.
//   eight sums in FP64, every term the exact product of two f32 samples: st = SUM T, ss = SUM S, stt = SUM T*T, sss = SUM S*S,
//              sts = SUM T*S, gxx = SUM Sgx*Sgx, gxy = SUM Sgx*Sgy, gyy = SUM Sgy*Sgy.  Term k joins partial k mod 64 in increasing k; the
//              64 partials fold by p[l] += p[l + m], l < m, for m = 32, 16, 8, 4, 2, 1 (the order of section 9 for sums that are not the
//              reference's).
//   ncc        FP64, one rounding per operation: nd = (double)n, a = nd*stt - st*st, b = nd*sss - ss*ss, c = nd*sts - st*ss;
//              a > 0 && b > 0: (float)clamp(c / sqrt(a*b), -1, 1), else 0.
//   min_eig    d = gxx - gyy, e = ((gxx + gyy) - sqrt(d*d + 4.0*(gxy*gxy))) / 2.0, (float)max(e, 0).
//
// One wavefront per feature.  Lane l owns window samples l, l + 64, ...: its FP64 partials ARE partials l of the rule, they live in
// registers and fold by cross-lane exchange; only the pairwise sum goes through LDS, in numpy's order.
//
// The FP64 division and square root are the compiler's expansions, which are built from FP64 fused multiply-adds and are correctly
// rounded as a whole; tests/test_host_and_abi.py allows a kernel those OR the FMAs of IEEE f32 divisions, by its symbol's name -- this
// one computes an eigenvalue and says so.  The residue's f32 quotient is therefore taken as (float)((double)s / (double)n): the same
// bits as s / (float)n (rounding a 53-bit quotient of two f32 once more to 24 bits cannot change it, 53 >= 2 * 24 + 2) without an f32
// division expansion; residue_mean keeps the compiler from narrowing it back.
//
// Bilinear, make_bilinear, sample, pairwise_block and pairwise_sum are the tracker's, from track_primitives.h: the single copy, moved
// there verbatim with the device assembly of this file compared before and after.
#include <cstdlib>

#include "klt_internal.h"
#include "track_primitives.h"

#pragma clang fp contract(off)

namespace quality_kernels {

// s / (float)n as an IEEE f32 quotient, through FP64 (see the head of the file).  The empty asm makes the quotient's operand opaque: the
// compiler would otherwise narrow fptrunc(fdiv(fpext s, fpext n)) back to the f32 division and its f32 FMA expansion.
__device__ __forceinline__ float residue_mean(float s, int n)
{
    double sd = (double)s;
    asm volatile("" : "+v"(sd));
    return (float)(sd / (double)n);
}

// the 64 partials of the rule, one per lane, folded into lane 0: p[l] += p[l + m], l < m, m = 32 .. 1 (lanes l >= m hold values nobody reads)
__device__ __forceinline__ double fold64(double p)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_down(p, m);
    return p;
}

// 0 <= v < limit, false for NaN and the infinities; to be asked before v is converted to int
__device__ __forceinline__ bool inside(float v, int limit) { return v >= 0.f && v < (float)limit; }

__device__ __forceinline__ bool window_fits(const Bilinear &b, int hw, int nc, int nr)
{
    return b.ix - hw >= 0 && b.iy - hw >= 0 && b.ix + hw + 2 <= nc && b.iy + hw + 2 <= nr;
}

// One feature per wavefront.  MAXK: window samples per lane; WCT > 0: window size known at compile time, WCT == 0: any odd window up to 31
template <int MAXK, int WCT, bool BATCH>
__global__ __launch_bounds__(64) void quality_eigen_kernel(QualityArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= a.n) return;
    QualityPair pr;
    if (BATCH) {
        typedef const __attribute__((address_space(4))) QualityPair *cptr;
        const cptr c = (cptr)(a.pairs + blockIdx.y);
        pr.i1 = c->i1; pr.i2 = c->i2; pr.gx2 = c->gx2; pr.gy2 = c->gy2;
        pr.in = c->in; pr.out = c->out; pr.q = c->q;
    } else {
        pr = a.one;
    }
    const int w = WCT > 0 ? WCT : a.window, n = w * w, hw = w / 2;
    const int nc = a.ncols, nr = a.nrows;
    const klt_feat fi = pr.in[f], fo = pr.out[f];
    f32x4 *const dst = reinterpret_cast<f32x4 *>(pr.q + f);

    bool measured = fi.val >= 0 && fo.val == KLT_TRACKED &&
                    inside(fi.x, nc) && inside(fi.y, nr) && inside(fo.x, nc) && inside(fo.y, nr);
    Bilinear b1, b2;
    if (measured) {
        b1 = make_bilinear(fi.x, fi.y);
        b2 = make_bilinear(fo.x, fo.y);
        measured = window_fits(b1, hw, nc, nr) && window_fits(b2, hw, nc, nr);
    }
    if (!measured) {
        if (lane == 0) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};           // (0, 0, 0, val = 0)
            *dst = zero;
        }
        return;
    }

    const size_t base1 = (size_t)(b1.iy - hw) * nc + (b1.ix - hw), base2 = (size_t)(b2.iy - hw) * nc + (b2.ix - hw);
    double st = 0., ss = 0., stt = 0., sss = 0., sts = 0., gxx = 0., gxy = 0., gyy = 0.;
#pragma unroll
    for (int kk = 0; kk < MAXK; kk++) {
        const int k = lane + 64 * kk;
        if (k < n) {
            const int off = (k / w) * nc + (k % w);
            const float t = sample<KLT_PIX_STRIDE>(pr.i1 + KLT_PIX_STRIDE * (base1 + off), nc, b1);
            const float s = sample<KLT_PIX_STRIDE>(pr.i2 + KLT_PIX_STRIDE * (base2 + off), nc, b2);
            const float sx = sample<KLT_PIX_STRIDE>(pr.gx2 + KLT_PIX_STRIDE * (base2 + off), nc, b2);
            const float sy = sample<KLT_PIX_STRIDE>(pr.gy2 + KLT_PIX_STRIDE * (base2 + off), nc, b2);
            lds[k] = fabsf(t - s);
            const double td = (double)t, sd = (double)s, sxd = (double)sx, syd = (double)sy;
            st = st + td;
            ss = ss + sd;
            stt = stt + td * td;
            sss = sss + sd * sd;
            sts = sts + td * sd;
            gxx = gxx + sxd * sxd;
            gxy = gxy + sxd * syd;
            gyy = gyy + syd * syd;
        }
    }
    __syncthreads();
    const float rsum = pairwise_sum<3>(lds, n, lane);       // valid in lane 0
    st = fold64(st); ss = fold64(ss); stt = fold64(stt); sss = fold64(sss); sts = fold64(sts);
    gxx = fold64(gxx); gxy = fold64(gxy); gyy = fold64(gyy);
    if (lane != 0) return;

    const float residue = residue_mean(rsum, n);

    const double nd = (double)n;
    const double p1 = nd * stt, p2 = st * st, p3 = nd * sss, p4 = ss * ss, p5 = nd * sts, p6 = st * ss;
    const double ca = p1 - p2, cb = p3 - p4, cc = p5 - p6;
    float ncc = 0.f;
    if (ca > 0. && cb > 0.) {
        const double ab = ca * cb;
        double v = cc / sqrt(ab);
        if (v < -1.) v = -1.;
        if (v > 1.) v = 1.;
        ncc = (float)v;
    }

    const double d = gxx - gyy;
    const double dd = d * d, xy = gxy * gxy;
    const double rad = dd + 4.0 * xy;
    const double e = ((gxx + gyy) - sqrt(rad)) / 2.0;
    const float min_eig = e > 0. ? (float)e : 0.f;

    const f32x4 rec = {residue, ncc, min_eig, __int_as_float(1)};
    *dst = rec;
}

template <bool BATCH>
static int launch_quality_t(hipStream_t s, const QualityArgs &a)
{
    const int n = a.window * a.window;
    if (a.window < 3 || !(a.window & 1) || n > 1024) return -1;
    const unsigned lds = (unsigned)(track_npad(n) * sizeof(float));
    const dim3 grid(a.n, BATCH ? a.npairs : 1), block(64);
    const TrackWindowClass wc = track_window_class(a.window);
    for_window_class(wc.maxk, wc.wct, [&](auto maxk, auto wct) {
        klt_launch((quality_eigen_kernel<maxk.value, wct.value, BATCH>), grid, block, lds, s, a);
    });
    return 0;
}

}  // namespace quality_kernels

// The quality launch (klt_track_quality_async / klt_track_quality_batch_async).  Returns -1 for an unsupported window.
int launch_track_quality(hipStream_t s, const QualityArgs &a)
{
    if (a.n <= 0) return 0;
    if (a.pairs) return a.npairs > 0 ? quality_kernels::launch_quality_t<true>(s, a) : 0;
    return quality_kernels::launch_quality_t<false>(s, a);
}
