// Prints what plan_track (pyfeaturetrack_amd/csrc/track_plan.h) answers for the requests on stdin: tests/test_track_plan_rule.py compiles
// this with g++ and holds the answers against the Python restatements of the rule.  No HIP, no GPU.
//   <window> <n> <batched> <npairs> <fb> <guess> <light> <tree_sums> <variant> <order> <order_chunk> <grad7> <all_compact> <lazy_form>
// One line of `field=value` pairs per request, every field of the plan (refusal: `-` or the text with `_` for its blanks).
#include <cstdio>
#include <string>

#include "track_plan.h"

int main()
{
    TrackRequest q = {};
    int batched, fb, guess, light, tree, order, grad7, compact;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &q.window, &q.n, &batched, &q.npairs, &fb, &guess, &light, &tree, &q.variant, &order,
                 &q.order_chunk, &grad7, &compact, &q.lazy_form) == 14) {
        q.batched = batched; q.fb = fb; q.guess = guess; q.light = light; q.tree_sums = tree; q.order = order; q.grad7 = grad7; q.all_compact = compact;
        const TrackPlan p = plan_track(q);
        std::string refusal = p.refusal ? p.refusal : "-";
        for (char &ch : refusal)
            if (ch == ' ') ch = '_';
        printf("launch=%d refusal=%s family=%d rule=%d batched=%d fb=%d guess=%d tree=%d lazy=%d entry=%d lazy_capable=%d need_records=%d maxk=%d wct=%d "
               "fpw=%d gx=%u gy=%u lds=%zu uses_order=%d light_path=%d\n", (int)p.launch, refusal.c_str(), p.family, p.rule, (int)p.batched, (int)p.fb,
               (int)p.guess, (int)p.tree, (int)p.lazy, (int)p.entry, (int)p.lazy_capable, (int)p.need_records, p.maxk, p.wct, p.fpw, p.gx, p.gy, p.lds,
               (int)p.uses_order, p.light_path);
    }
    return feof(stdin) ? 0 : 2;
}
