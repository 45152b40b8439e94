// Which kernel a tracker launch gets, with which grid and how much LDS, and what it asks of level 0: one request type, one plan type, one
// planner.  Plain C++17 -- no HIP in here -- so that the rule is checked where there is no GPU (tests/test_track_plan_rule.py).  The launcher
// (launch_track, track_kernels.hip) executes a plan and decides nothing; the host (launch_pairs, api_track.hip) makes one plan per launch and
// reads everything off it.
#pragma once
#include <cstddef>

// 16-byte aligned sub-arrays: the five product arrays of a window of n samples in LDS
constexpr int track_npad(int n) { return (n + 3) & ~3; }
constexpr size_t track_lds_bytes(int n) { return 5 * (size_t)track_npad(n) * sizeof(float); }

// The window classes of the one-feature-per-wavefront kernels: maxk window samples per lane; wct the window size where it is known at
// compile time (7 and 15), 0 for any other window of n = window * window <= 1024 samples
struct TrackWindowClass {
    int maxk, wct;
};
constexpr TrackWindowClass track_window_class(int window)
{
    const long long n = (long long)window * window;
    if (window == 7) return {1, 7};
    if (window == 15) return {4, 15};
    return {n <= 64 ? 1 : n <= 128 ? 2 : n <= 256 ? 4 : n <= 512 ? 8 : 16, 0};
}

// features x pairs from which a 7x7 launch takes four features per wavefront (shorter lists keep one: with a few hundred features the launch
// is pure latency, which four features in lock step lengthen)
constexpr long long TRACK_QUAD7_MIN = 2048;
// LDS floats of the lazy 7x7 kernels at level 0 (track_kernels.hip holds static_asserts against its own constants): per feature the patch
// with its two filtered planes; per wavefront the two patches of the fused entry phase with the image values set aside
constexpr int TRACK_LAZY_FLOATS = 464, TRACK_LAZY_ENTRY_FLOATS = 2528;

// What the decision depends on, and nothing else
struct TrackRequest {
    int window, n;
    bool batched;           // a table of pair descriptors (klt_track*_batch_async) ...
    int npairs;             // ... of so many pairs
    bool fb, guess;         // the forward-backward check, a motion prior
    bool light;             // klt_set_light_params mode 1
    bool tree_sums;         // KLT_OPT_TRACK_TREE_SUMS
    int variant;            // KLT_OPT_TRACK_VARIANT: 0 = always one feature per wavefront
    bool order;             // an XCD-aware feature order is offered (KLT_OPT_TRACK_XCD_ORDER, n >= 64, not light) ...
    int order_chunk;        // ... of so many features per XCD
    bool grad7;             // 7-tap gradient filters (merged_grad_ok)
    bool all_compact;       // every slot of the launch holds a compact level-0 image
    int lazy_form;          // KLT_OPT_TRACK_LAZY_FORM
};

enum TrackFamily { TRACK_FAMILY_WAVE, TRACK_FAMILY_QUAD7, TRACK_FAMILY_QUAD15 };   // track_kernel / track_light_kernel, track_kernel_quad<7> / track_light_quad, track_kernel_quad<15>
enum TrackRule { TRACK_RULE_PLAIN, TRACK_RULE_LIGHT };                             // track_kernels.hip, track_light_kernels.hip

// The whole answer
struct TrackPlan {
    bool launch;            // false: nothing to track, nothing goes out
    const char *refusal;    // null, or why the launch cannot be made
    int family, rule;       // TrackFamily, TrackRule
    bool batched, fb, guess;
    bool tree;              // the instantiation that adds its sums by a butterfly in registers
    bool lazy;              // level 0 is read as compact images (TrackLazyArgs) ...
    bool entry;             // ... with the template's and the first footprint's gradients in one fused phase
    bool lazy_capable;      // the launch has a lazy form: it leaves its mark on the slots it reads, and records made for it are not held against them
    bool need_records;      // slots without level-0 records get them before the launch
    int maxk, wct;          // the window class
    int fpw;                // features per wavefront
    unsigned gx, gy;        // grid
    size_t lds;             // dynamic LDS bytes
    bool uses_order;        // the kernels take the feature order (refreshed by track_order_kernel when the arguments ask for it)
    int light_path;         // what klt_track_light_path reports: 0 not a gain / bias launch, 1 wave kernel, 2 quad kernel
};

// The launches that may have a lazy form at all.  (A single-pair launch outside them has its level-0 records made slot by slot while the pair
// is checked: check_pair, api_track.hip.)
constexpr bool track_lazy_rule(bool fb, bool guess, bool light) { return !fb && !guess && !light; }

inline TrackPlan plan_track(const TrackRequest &q)
{
    TrackPlan p = {};
    const int ny = q.batched ? q.npairs : 1;
    const TrackWindowClass wc = track_window_class(q.window);
    p.batched = q.batched; p.fb = q.fb; p.guess = q.guess;
    p.maxk = wc.maxk; p.wct = wc.wct;
    p.rule = q.light ? TRACK_RULE_LIGHT : TRACK_RULE_PLAIN;
    // 7x7: four features per wavefront from TRACK_QUAD7_MIN features in the launch.  15x15: the quad kernel, which has no gain / bias form.
    // Variant 0 forces the wave kernels: the plain fallback the parity tests compare the quad kernels with
    const bool quad7 = q.variant != 0 && wc.wct == 7 && (long long)q.n * ny >= TRACK_QUAD7_MIN;
    p.family = quad7 ? TRACK_FAMILY_QUAD7 : q.variant != 0 && wc.wct == 15 && !q.light ? TRACK_FAMILY_QUAD15 : TRACK_FAMILY_WAVE;
    p.fpw = p.family == TRACK_FAMILY_QUAD7 ? 4 : 1;
    // tree sums: the plain quad kernels alone (the forward-backward check uses the reference-order sums)
    p.tree = q.tree_sums && !q.fb && !q.light && p.family != TRACK_FAMILY_WAVE;
    // lazy: the plain 7x7 quad kernel with the reference-order sums under 7-tap gradient filters, on slots that all hold a compact image
    p.lazy_capable = track_lazy_rule(q.fb, q.guess, q.light) && quad7 && !q.tree_sums && q.n > 0 && ny > 0 && q.grad7;
    p.lazy = p.lazy_capable && q.all_compact;
    p.entry = p.lazy && q.lazy_form != 0;
    p.need_records = !p.lazy;
    p.launch = q.n > 0 && ny > 0;
    if (!p.launch) return p;
    if ((long long)q.window * q.window > 1024) p.refusal = "unsupported window size";
    if (q.batched && q.fb && q.guess) p.refusal = "no batched launch takes a motion prior and the forward-backward check together";
    // the gain / bias kernels take their features in list order
    p.uses_order = q.order && !q.light;
    p.light_path = !q.light ? 0 : p.family == TRACK_FAMILY_QUAD7 ? 2 : 1;
    // with an order: eight chunks of features, one per XCD, each rounded up to whole wavefronts
    p.gx = (unsigned)(p.uses_order ? 8 * ((q.order_chunk + p.fpw - 1) / p.fpw) : (q.n + p.fpw - 1) / p.fpw);
    p.gy = (unsigned)ny;
    // LDS: the product arrays of a wavefront's features (none with tree sums); lazy: those or, at level 0, the features' patches (the larger
    // of the two), or the two patches of the fused entry phase (which the patches of the Newton loop's recomputations fit under)
    constexpr size_t lazy_lds = 4 * sizeof(float) * (TRACK_LAZY_FLOATS > 5 * track_npad(49) ? TRACK_LAZY_FLOATS : 5 * track_npad(49));
    constexpr size_t entry_lds = sizeof(float) * TRACK_LAZY_ENTRY_FLOATS;
    static_assert(entry_lds >= lazy_lds && entry_lds <= 10240, "sixteen wavefronts per CU");
    p.lds = p.entry ? entry_lds : p.lazy ? lazy_lds : p.tree || p.refusal ? 0 : p.fpw * track_lds_bytes(q.window * q.window);
    return p;
}
