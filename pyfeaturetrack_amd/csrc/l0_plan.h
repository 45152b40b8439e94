// Which kernel a level-0 (or gradient) launch gets, and in which form: one plan type, one planner.  Plain C++17 -- no HIP in here -- so that
// the rule is checked where there is no GPU (tests/test_l0_plan_rule.py).  The launcher (launch_smooth_grad, pyramid_kernels.hip) executes
// a plan and decides nothing; the callers (api_frames.hip, api_select.hip) make one plan per launch and read everything off it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "klt_gpu.h"

// FP64 taps in the order scipy.ndimage.correlate1d consumes them (i.e. the convolve.py taps reversed,
// convolve1d does `weights[::-1]`), plus the symmetry class its inner loop switches on.
struct Taps {
    double k[KLT_MAX_KERNEL_WIDTH];
    int n;
    int sym;   // +1 symmetric, -1 antisymmetric, 0 neither
};

constexpr int KLT_MAX_BATCH = 32;   // frames per fused pyramid launch (pointer tables travel in the kernarg segment)

#if defined(__HIPCC__)
#define KLT_RULE_HD __host__ __device__
#else
#define KLT_RULE_HD
#endif

// May a level-0 kernel read the frame at `addr` (rows of `ncols` elements of `elem_bytes`, no padding) four elements to a load?  Only
// where every quad of every row then sits on a multiple of its own size: a width divisible by 4 AND a first byte on a multiple of
// 4 * elem_bytes (4 for u8 frames, 16 for f32 frames).  An adopted frame (klt_slot_adopt_u8) may start at any byte, so the width alone
// does not tell; frames that miss either half are read element by element.  The one home of this rule: every raw-frame quad load of
// pyramid_kernels.hip asks here, per frame of a batch (tests/test_l0_plan_rule.py sweeps it without a GPU).
KLT_RULE_HD inline bool raw_quads_aligned(uintptr_t addr, int ncols, int elem_bytes)
{
    return ncols % 4 == 0 && addr % (uintptr_t)(4 * elem_bytes) == 0;
}

// What the decision depends on, and nothing else
struct L0Request {
    int ncols, nrows;       // the largest entry (grid extent)
    int batch;              // entries of the launch
    int kind;               // 0 = u8 frame + smoothing, 1 = f32 frame + smoothing, 2 = f32 image, gradients only, 3 = u8 image, gradients only
    bool uniform;           // every entry has the launch's own size (no dim_c / dim_r)
    const Taps *smooth, *ggauss, *gderiv, *reduce;
    int ss;                 // subsampling
    bool fuse_hreduce;      // KLT_OPT_FUSED_HREDUCE
    int l0_stream;          // KLT_OPT_L0_STREAM: 0 / 1 = 64-column strips / 2 = 128-column strips where they apply
    int lean_form_opt;      // KLT_OPT_L0_LEAN_FORM: 1 = a lean launch takes the wave form where it applies
    bool want_hred;         // the caller has levels >= 1 and a fused reduction kernel to consume H1
    bool want_lean;         // the caller would take the lean form (honoured only where a streaming geometry is taken)
};

// Geometry of the kernels (pyramid_kernels.hip holds static_asserts against its own constants)
constexpr int L0_TILE_W = 64, L0_TILE_H = 16;                       // output tile of smooth_grad_kernel; 64 is the register-blocked tile's width too
constexpr int L0S_TW = 64, L0S_SB = 32, L0W_TW = 128, L0W_SB = 16;  // streaming: 64-column strips in 32-row bands, 128-column strips in 16-row bands
constexpr int L0_WAVE_COLS = 232, L0_WAVE_WAVES = 4;                // wave form: output columns of a strip, wavefronts per workgroup
// Workgroups a launch needs to take a streaming geometry: two rounds of the 1024 resident slots (256 CUs x 4) for the narrow strips; the wide
// strips' grid of sixteen 1080p frames is 15 x 9 x 16 = 2160 at their segment height, so the same bound holds for them
constexpr long long L0S_MIN_WGS = 2048, L0W_MIN_WGS = 2048;

// Experiment hooks with their defaults: KLT_RB_TH (16 or 32: the tile height; 0: by the launch's pixel count), KLT_L0_SEG (segment height; a banded
// geometry takes it only where its band height divides it, the wave form takes any; 0: each form's own), KLT_L0_WIDE_WGS (the wide strips' grid bound)
struct L0Tuning {
    int rb_th = 0, l0_seg = 0;
    long long wide_wgs = L0W_MIN_WGS;
};

// ... as the library reads them: from the environment, once per process
inline const L0Tuning &l0_tuning_from_env()
{
    static const L0Tuning t = [] {
        L0Tuning u;
        if (const char *v = getenv("KLT_RB_TH")) u.rb_th = atoi(v);
        if (const char *v = getenv("KLT_L0_SEG")) u.l0_seg = atoi(v);
        if (const char *v = getenv("KLT_L0_WIDE_WGS")) { if (atoll(v) > 0) u.wide_wgs = atoll(v); }
        return u;
    }();
    return t;
}

enum L0Family { L0_FAMILY_TILED_LDS, L0_FAMILY_RB_TILE, L0_FAMILY_BANDED, L0_FAMILY_WAVE };   // smooth_grad_kernel, _rb, _stream, _lean_wave

// The whole answer
struct L0Plan {
    int kind;               // the request's (the launcher picks the instantiation's input type by it)
    int path;               // the KLT_L0_* code klt_level0_path reports
    bool hred;              // the first reduction's horizontal pass goes out with this launch (H1 planes)
    bool lean;              // no gradients, no records: the smoothed image to the compact planes
    int lean_form;          // 0 not lean, 1 banded, 2 wave
    bool zc;                // the centre-elided instantiation (corr_regs<..., ZC>)
    int family;             // L0Family
    int tile_rows;          // register-blocked and tiled-LDS kernels: 16 / 32
    int strip, band, seg;   // streaming kernels: strip width, band height (0: the wave form has none), segment height
    int nstrips, nsegs;     // ... and how many of each a frame has
    int units;              // wave form: strips x segments x frames, four to a workgroup
    unsigned gx, gy, gz;    // grid
    int block;
    size_t lds;             // dynamic LDS bytes
};

inline size_t smooth_grad_lds_bytes(int rs /* smoothing radius; -1: no smoothing stage */, int R)
{
    const int IW = L0_TILE_W + 2 * R, IH = L0_TILE_H + 2 * R, RW = IW + 2 * rs, RH = IH + 2 * rs;
    const int ab = rs >= 0 ? RH * RW + RH * IW : 0, de = 2 * IH * L0_TILE_W;
    return sizeof(float) * (size_t)((ab > de ? ab : de) + IH * IW);
}

// The taps the register-blocked and streaming kernels are compiled for: 7 gradient taps, Gaussian symmetric and derivative antisymmetric,
// and (smooth given: the smoothing kinds) 5 or 9 symmetric smoothing taps
inline bool l0_taps_specialised(const Taps *smooth, const Taps &ggauss, const Taps &gderiv)
{
    return ggauss.sym == 1 && gderiv.sym == -1 && ggauss.n == 7 && gderiv.n == 7 &&
           (!smooth || (smooth->sym == 1 && (smooth->n == 5 || smooth->n == 9)));
}

// The derivative taps' centre is +0.0 and every sample the two derivative passes see is >= +0 (a u8 frame, smoothing and Gaussian
// taps without sign bits): corr_regs<..., ZC> may drop the centre product
inline bool l0_deriv_centre_elidable(const L0Request &q)
{
    auto sign_free = [](const Taps &t) {
        for (int i = 0; i < t.n; i++)
            if (std::signbit(t.k[i]) || !std::isfinite(t.k[i])) return false;
        return true;
    };
    uint64_t centre;
    std::memcpy(&centre, &q.gderiv->k[q.gderiv->n / 2], sizeof(centre));
    return q.kind == 0 && centre == 0 && sign_free(*q.smooth) && sign_free(*q.ggauss);
}

inline L0Plan plan_level0(const L0Request &q, const L0Tuning &tune)
{
    auto cdiv = [](int a, int b) { return (unsigned)((a + b - 1) / b); };
    const bool smooth = q.kind < 2;
    L0Plan p = {};
    p.kind = q.kind;
    p.block = 256;
    p.gz = (unsigned)q.batch;
    if (!l0_taps_specialised(smooth ? q.smooth : nullptr, *q.ggauss, *q.gderiv)) {
        // taps of any count: the LDS-tiled kernel (asymmetric smoothing taps never get here: fused_smooth_ok)
        p.path = KLT_L0_TILED_LDS; p.family = L0_FAMILY_TILED_LDS; p.tile_rows = L0_TILE_H;
        p.gx = cdiv(q.ncols, L0_TILE_W); p.gy = cdiv(q.nrows, L0_TILE_H);
        const int R = (q.ggauss->n > q.gderiv->n ? q.ggauss->n : q.gderiv->n) / 2;
        p.lds = smooth_grad_lds_bytes(smooth ? q.smooth->n / 2 : -1, R);
        return p;
    }
    // The register-blocked kernels take the 32-row tile for launches of a million pixels; smaller ones take the 16-row tile so that the
    // grid still covers the chip
    const bool tall = tune.rb_th ? tune.rb_th == 32 : (long long)q.ncols * q.nrows * q.batch >= 1000000;
    // The fused horizontal reduction: the smoothing kinds, tall tiles, subsampling 4 with 21 taps, frames tall enough that the vertical pass
    // needs a single reflection
    p.hred = q.want_hred && q.fuse_hreduce && smooth && tall && q.ss == 4 && q.reduce->sym == 1 && q.reduce->n == 21 && q.nrows >= 64 && q.ncols >= 64;
    p.family = L0_FAMILY_RB_TILE; p.tile_rows = tall ? 32 : 16;
    p.gx = cdiv(q.ncols, L0_TILE_W); p.gy = cdiv(q.nrows, p.tile_rows);
    p.path = p.hred ? KLT_L0_RB32_HRED : tall ? KLT_L0_RB32 : KLT_L0_RB16;
    if (!p.hred) return p;
    // Streaming is considered only with the fused reduction.  Segment height per geometry: the fastest of each one's cfg-2 sweep
    // (profiles/README.md).  Wide strips (KLT_OPT_L0_STREAM 2): frames of two wide strips or more and a grid of two rounds of the resident
    // slots at their own segment height; launches that miss either fall through to the narrow strips' rule (frames of two strips or more,
    // the same two rounds), and from there to the tile, whose 32-row tiles fill the chip (one 4K frame, 1080p batches below 10)
    auto seg_of = [&](int band, int own) { return tune.l0_seg > 0 && tune.l0_seg % band == 0 ? tune.l0_seg : own; };
    const int shw = seg_of(L0W_SB, 128), sh = seg_of(L0S_SB, 160);
    const long long gw = (long long)cdiv(q.ncols, L0W_TW) * cdiv(q.nrows, shw) * q.batch;
    const long long gs = (long long)cdiv(q.ncols, L0S_TW) * cdiv(q.nrows, sh) * q.batch;
    const bool wide = q.l0_stream == 2 && q.ncols >= 2 * L0W_TW && gw >= tune.wide_wgs;
    if (!wide && !(q.l0_stream && q.ncols >= 2 * L0S_TW && gs >= L0S_MIN_WGS)) return p;
    p.family = L0_FAMILY_BANDED; p.tile_rows = 0;
    p.strip = wide ? L0W_TW : L0S_TW; p.band = wide ? L0W_SB : L0S_SB; p.seg = wide ? shw : sh;
    p.gx = p.nstrips = cdiv(q.ncols, p.strip); p.gy = p.nsegs = cdiv(q.nrows, p.seg);
    // (the centre-tap elision needs a u8 frame: no f32 instantiation of it.  The lean form has no derivative pass: one instantiation per
    // input type and tap count, reported under the code the full launch would get)
    const bool elidable = l0_deriv_centre_elidable(q);
    p.path = wide ? (elidable ? KLT_L0_STREAM_WIDE_NO_CENTRE : KLT_L0_STREAM_WIDE) : (elidable ? KLT_L0_STREAM_NO_CENTRE : KLT_L0_STREAM);
    p.lean = q.want_lean;
    p.zc = elidable && !p.lean;
    p.lean_form = p.lean ? 1 : 0;
    // A lean launch takes the wave form where it is asked for and applies: frames of >= 256 columns and at least one vertical window high
    // (one reflection brings every index of a strip inside), all of one size.  Its segment height: the fastest of its sweep
    if (p.lean && q.lean_form_opt == 1 && q.uniform && q.ncols >= 256 && q.nrows >= q.smooth->n) {
        p.family = L0_FAMILY_WAVE; p.lean_form = 2;
        p.strip = L0_WAVE_COLS; p.band = 0; p.seg = tune.l0_seg > 0 ? tune.l0_seg : KLT_L0_LEAN_WAVE_SEG;
        p.nstrips = cdiv(q.ncols, p.strip); p.nsegs = cdiv(q.nrows, p.seg); p.units = p.nstrips * p.nsegs * q.batch;
        p.gx = cdiv(p.units, L0_WAVE_WAVES); p.gy = p.gz = 1;
        p.block = 64 * L0_WAVE_WAVES;
    }
    return p;
}
