// Stage timing of the level-0 kernel: includes the product source with KLT_STAGE_CLOCKS and prints, for 64 workgroups of one
// tile row, the wall-clock ticks (100 MHz) spent between the stage marks.  `T`: the tiled kernel with the fused reduction, `s`: the
// streaming kernel, `w`: the streaming kernel on 128-column strips (per-stage ticks summed over the bands of one segment), all on 16 1080p u8 frames into planes of pixel records
// as at cfg-2 (`p`, the tiled kernel without the fused reduction, also writes the compact image copy the build then asks for).  Build (from the repo root):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -DKLT_STAGE_CLOCKS -Iinclude -Ipyfeaturetrack_amd/csrc tools/mb/l0_stages.hip -o tools/mb/l0_stages
// `l` / `n`: the lean banded kernel on wide / narrow strips (into compact planes), `v`: the lean wave form (time per launch only).
// Without -DKLT_STAGE_CLOCKS it launches the product kernels unmarked and prints the time per launch only (the program a counter pass
// runs; built as tools/mb/l0_plain).
#include "../../pyfeaturetrack_amd/csrc/pyramid_kernels.hip"
#include <cstdio>
#include <cmath>
#include <vector>

thread_local hipEvent_t g_klt_stamp_start, g_klt_stamp_stop;      // (defined by the library's api_context.hip; klt_launch reads them)

static void gauss_taps(Taps &g, Taps &d, double sigma, int n)
{
    const int h = n / 2;
    double sg = 0, sd = 0;
    for (int i = -h; i <= h; i++) { g.k[i + h] = exp(-i * i / (2 * sigma * sigma)); d.k[i + h] = -i * g.k[i + h]; sg += g.k[i + h]; sd -= i * d.k[i + h]; }
    for (int i = 0; i < n; i++) { g.k[i] /= sg; d.k[i] /= sd; }
    g.n = d.n = n; g.sym = 1; d.sym = -1;
}

int main(int argc, char **argv)
{
    const bool reduce = argc > 1 && argv[1][0] == 'r';
    const bool level = false;
    const int nc = 1920, nr = 1080;
    SmoothGradArgs a = {};
    Taps dummy;
    gauss_taps(a.smooth, dummy, 0.7, 5);
    gauss_taps(a.ggauss, a.gderiv, 1.0, 7);
    a.ncols = nc; a.nrows = nr; a.R = 3;
    std::vector<uint8_t> h((size_t)nc * nr);
    for (size_t i = 0; i < h.size(); i++) h[i] = (uint8_t)((i * 2654435761u) >> 24);
    // `l` / `n`: the lean form (KLT_OPT_L0_LAZY_GRAD) of the wide / narrow streaming kernel: stages load, hsm, vsm and (as "hgrad") the
    // plane stores with the horizontal reduction; `v`: the lean wave form (no stage marks: time per launch only)
    const char mode = argc > 1 ? argv[1][0] : ' ';
    const bool wave = mode == 'v';
    const bool lean_mode = mode == 'l' || mode == 'n' || wave;
    const bool wide = mode == 'w' || mode == 'l' || wave;
    const bool tiled16 = mode == 'T', stream = wide || mode == 's' || mode == 'n';
    const int B = tiled16 || stream ? 16 : 2;
    const bool plain = argc > 1 && argv[1][0] == 'p';      // the kernel without the fused horizontal reduction
    float *cimg[KLT_MAX_BATCH], *dst[KLT_MAX_BATCH];
    for (int b = 0; b < B; b++) {
        uint8_t *raw; float *rec;
        hipMalloc(&raw, h.size()); hipMalloc(&rec, 4 * KLT_PIX_STRIDE * h.size()); hipMalloc(&cimg[b], 4 * h.size()); hipMalloc(&dst[b], 4 * h.size());
        hipMemcpy(raw, h.data(), h.size(), hipMemcpyHostToDevice);
        a.raw[b] = raw; a.rec[b] = rec; a.cimg[b] = plain || lean_mode ? cimg[b] : nullptr;
    }
    PyrReduceArgs pr = {};
    gauss_taps(pr.taps, dummy, 3.6, 21);
    pr.src_nc = nc; pr.src_nr = nr; pr.dst_nc = nc / 4; pr.dst_nr = nr / 4; pr.ss = 4; pr.log2ss = 2;
    for (int b = 0; b < 2; b++) { pr.src[b] = cimg[b]; pr.dst[b] = dst[b]; }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    a.reduce = pr.taps; a.h1_nc = nc / 4;
    for (int b = 0; b < B; b++) { float *h1; hipMalloc(&h1, 4 * (size_t)nr * (nc / 4)); a.h1[b] = h1; }
    // the launch's plan, as the library makes it (the mode sets the options and the wishes; the experiment hooks are the library's)
    const L0Request q = {nc, nr, B, 0, true, &a.smooth, &a.ggauss, &a.gderiv, &a.reduce, 4, true, wide ? 2 : stream ? 1 : 0, wave ? 1 : 0, !plain, lean_mode};
    const L0Plan plan = plan_level0(q, l0_tuning_from_env());
    if (plan.hred == plain || plan.lean != lean_mode || plan.lean_form != (wave ? 2 : lean_mode ? 1 : 0) ||
        (stream && !wave && (plan.family != L0_FAMILY_BANDED || plan.strip != (wide ? 128 : 64)))) {
        printf("the plan is not the form asked for\n");
        return 1;
    }
    auto go = [&]() {
        if (reduce) launch_pyr_reduce(0, pr, 2);
        else launch_smooth_grad(0, a, plan);
    };
    for (int rep = 0; rep < 3; rep++) go();
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int rep = 0; rep < 20; rep++) go();
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("kernel: %.2f us per launch\n", ms * 1000 / 20);
#ifndef KLT_STAGE_CLOCKS
    return 0;                                   // (built without the stage marks: the product kernels, for counter passes)
#else
    if (wave) return 0;
    long long clk[64 * 8];
    if (stream) {
        // g_stream_clk accumulated over every launch of this run (3 + 20): per launch, per band of 2048 output pixels (32 rows of a 64-column
        // strip, 16 of a 128-column one; the segment height is the plan's: the kernel's own, or KLT_L0_SEG as the library reads it)
        hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_stream_clk), sizeof(clk));
        const int sb = plan.band, seg = plan.seg, nb = plan.nstrips;
        const double per = 23.0 * (seg / sb);
        printf("ticks of 10 ns per band of 2048 output pixels (segment 1 of frame 0, %d rows, prologue share included)\nblock | load  hsm  vsm  hgrad vgrad | total\n", seg);
        double sum[5] = {};
        for (int b = 0; b < nb; b++) {
            const long long *c = clk + b * 8;
            double t = 0;
            for (int k = 0; k < 5; k++) { sum[k] += c[k] / per; t += c[k] / per; }
            printf("%4d | %5.0f %5.0f %5.0f %5.0f %5.0f | %6.0f\n", b, c[0] / per, c[1] / per, c[2] / per, c[3] / per, c[4] / per, t);
        }
        printf("mean | %5.0f %5.0f %5.0f %5.0f %5.0f | %6.0f\n", sum[0] / nb, sum[1] / nb, sum[2] / nb, sum[3] / nb, sum[4] / nb,
               (sum[0] + sum[1] + sum[2] + sum[3] + sum[4]) / nb);
        return 0;
    }
    hipMemcpyFromSymbol(clk, HIP_SYMBOL(g_stage_clk), sizeof(clk));
    long long t0 = clk[0];
    const int nrow = level ? 8 : reduce ? 15 : 30;
    for (int b = 0; b < nrow; b++) t0 = clk[b * 8] < t0 ? clk[b * 8] : t0;
    printf("ticks of 10 ns; tile row 8 of frame 0\nblock  start | load  hsm  vsm  hgrad vgrad | total\n");
    double tsum[5] = {};
    for (int b = 0; b < nrow; b++) {
        const long long *c = clk + b * 8;
        for (int k = 0; k < 5; k++) tsum[k] += c[k + 1] - c[k];
        if (reduce) printf("%4d %6lld | load %4lld  hpass %4lld  vpass %4lld | %5lld\n", b, c[0] - t0, c[1] - c[0], c[2] - c[1], c[5] - c[2], c[5] - c[0]);
        else printf("%4d %6lld | %4lld %4lld %4lld %4lld %4lld | %5lld\n", b, c[0] - t0, c[1] - c[0], c[2] - c[1], c[3] - c[2], c[4] - c[3], c[5] - c[4], c[5] - c[0]);
    }
    if (!reduce) printf("mean | %5.0f %5.0f %5.0f %5.0f %5.0f\n", tsum[0] / nrow, tsum[1] / nrow, tsum[2] / nrow, tsum[3] / nrow, tsum[4] / nrow);
    if (tiled16) return 0;
    static long long bc[8192 * 2];
    static unsigned hw[8192];
    hipMemcpyFromSymbol(bc, HIP_SYMBOL(g_block_clk), sizeof(bc));
    hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_block_hw), sizeof(hw));
    const int nb = level ? 8 * 17 * 2 : reduce ? 15 * 34 * 2 : 30 * 34 * 2;
    long long b0 = bc[0], b1 = 0;
    for (int i = 0; i < nb; i++) { if (bc[2 * i] < b0) b0 = bc[2 * i]; if (bc[2 * i + 1] > b1) b1 = bc[2 * i + 1]; }
    printf("first start -> last end: %lld ticks\n", b1 - b0);
    int hs[64] = {}, he[64] = {}; double dur[64] = {}; int nd[64] = {};
    for (int i = 0; i < nb; i++) {
        const int s = (int)((bc[2 * i] - b0) / 100), e = (int)((bc[2 * i + 1] - b0) / 100);
        hs[s < 63 ? s : 63]++; he[e < 63 ? e : 63]++; dur[s < 63 ? s : 63] += bc[2 * i + 1] - bc[2 * i]; nd[s < 63 ? s : 63]++;
    }
    printf("per microsecond: workgroups started / ended / mean duration (ticks) of those started\n");
    for (int t = 0; t < 40; t++) printf("%3d us: %5d %5d %7.0f\n", t, hs[t], he[t], nd[t] ? dur[t] / nd[t] : 0.0);
    // residency: which workgroups ran on each (xcc, se, sh, cu)
    static int cnt[8 * 256]; static long long lastend[8 * 256]; static long long firstend[8 * 256];
    for (int i = 0; i < 8 * 256; i++) { cnt[i] = 0; lastend[i] = 0; firstend[i] = 1 << 30; }
    for (int i = 0; i < nb; i++) {
        const unsigned h = hw[i] & 0xffff, x = (hw[i] >> 16) & 0x7;
        const int key = (int)x * 256 + (int)((h >> 8) & 0xff);       // cu_id[3:0] sh_id se_id[2:0]
        cnt[key]++;
        const long long e = bc[2 * i + 1] - b0;
        if (e > lastend[key]) lastend[key] = e;
        if (e < firstend[key]) firstend[key] = e;
    }
    int used = 0, hist[32] = {};
    for (int i = 0; i < 8 * 256; i++) if (cnt[i]) { used++; hist[cnt[i] < 31 ? cnt[i] : 31]++; }
    printf("CUs used %d; CUs by number of workgroups they ran:", used);
    for (int c = 0; c < 32; c++) if (hist[c]) printf("  %d wg: %d CUs", c, hist[c]);
    printf("\nper XCC: CUs, workgroups, mean first end, mean last end\n");
    for (int x = 0; x < 8; x++) {
        int c = 0, w = 0; double fe = 0, le = 0;
        for (int i = 0; i < 256; i++) if (cnt[x * 256 + i]) { c++; w += cnt[x * 256 + i]; fe += firstend[x * 256 + i]; le += lastend[x * 256 + i]; }
        if (c) printf("  xcc %d: %3d CUs %4d wgs  first end %.0f  last end %.0f\n", x, c, w, fe / c, le / c);
    }
    printf("xcc 0, per CU: id count firstend lastend\n");
    for (int i = 0; i < 256; i++) if (cnt[i]) printf("   %02x %2d %5lld %5lld\n", i, cnt[i], firstend[i], lastend[i]);
    // peak concurrency per CU: events
    return 0;
#endif
}
