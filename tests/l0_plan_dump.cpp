// Prints what plan_level0 (pyfeaturetrack_amd/csrc/l0_plan.h) answers for the requests on stdin: tests/test_l0_plan_rule.py compiles this
// with g++ and holds the answers against the Python restatements of the rule.  No HIP, no GPU.
//   T <name> <n> <sym> <k0> ... <kn-1>       defines a tap set (hex floats), in the order the library keeps them
//   R <ncols> <nrows> <batch> <kind> <uniform> <smooth> <ggauss> <gderiv> <reduce> <ss> <fuse_hreduce> <l0_stream> <lean_form_opt>
//     <want_hred> <want_lean> <rb_th> <l0_seg> <wide_wgs>      one request (tap sets by name, then the three tuning hooks; 0 = default)
//   Q <addr> <ncols> <elem_bytes>             raw_quads_aligned: may a frame at that address be read four elements to a load
// One line of `field=value` pairs per request, every field of the plan; one line `quads=0|1` per Q.
#include <cstdio>
#include <map>
#include <string>

#include "l0_plan.h"

int main()
{
    std::map<std::string, Taps> taps;
    char tag[8], name[4][64];
    while (scanf("%7s", tag) == 1) {
        if (tag[0] == 'T') {
            Taps t = {};
            if (scanf("%63s %d %d", name[0], &t.n, &t.sym) != 3 || t.n < 1 || t.n > KLT_MAX_KERNEL_WIDTH) return 2;
            for (int i = 0; i < t.n; i++)
                if (scanf("%la", &t.k[i]) != 1) return 2;
            taps[name[0]] = t;
            continue;
        }
        if (tag[0] == 'Q') {
            unsigned long long addr;
            int ncols, elem_bytes;
            if (scanf("%llu %d %d", &addr, &ncols, &elem_bytes) != 3) return 2;
            printf("quads=%d\n", (int)raw_quads_aligned((uintptr_t)addr, ncols, elem_bytes));
            continue;
        }
        L0Request q = {};
        L0Tuning tune;
        int uniform, fuse, want_hred, want_lean;
        long long wide_wgs;
        if (scanf("%d %d %d %d %d %63s %63s %63s %63s %d %d %d %d %d %d %d %d %lld", &q.ncols, &q.nrows, &q.batch, &q.kind, &uniform, name[0], name[1],
                  name[2], name[3], &q.ss, &fuse, &q.l0_stream, &q.lean_form_opt, &want_hred, &want_lean, &tune.rb_th, &tune.l0_seg,
                  &wide_wgs) != 18)
            return 2;
        if (wide_wgs > 0) tune.wide_wgs = wide_wgs;
        for (int i = 0; i < 4; i++)
            if (!taps.count(name[i])) return 3;
        q.uniform = uniform; q.fuse_hreduce = fuse; q.want_hred = want_hred; q.want_lean = want_lean;
        q.smooth = &taps[name[0]]; q.ggauss = &taps[name[1]]; q.gderiv = &taps[name[2]]; q.reduce = &taps[name[3]];
        const L0Plan p = plan_level0(q, tune);
        printf("kind=%d path=%d hred=%d lean=%d lean_form=%d zc=%d family=%d tile_rows=%d strip=%d band=%d seg=%d nstrips=%d nsegs=%d units=%d "
               "gx=%u gy=%u gz=%u block=%d lds=%zu\n", p.kind, p.path, (int)p.hred, (int)p.lean, p.lean_form, (int)p.zc, p.family, p.tile_rows, p.strip,
               p.band, p.seg, p.nstrips, p.nsegs, p.units, p.gx, p.gy, p.gz, p.block, p.lds);
    }
    return 0;
}
