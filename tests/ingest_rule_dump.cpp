// TEST INFRASTRUCTURE ONLY -- the host rules of the frame ingest path (csrc/ingest_rule.h) answered one question per input line, for
// tests/test_ingest_rule.py.  A stand-alone host program: built under the address and undefined-behaviour sanitizers, never loaded into
// anything.  Questions on stdin, answers on stdout, one line each:
//   E ncols nrows tiles_x tiles_y      -> equalisable_refusal: the refusal's text, or "ok"
//   S nrows tiles_y batch              -> the apply launch's split
//   L ncols nrows tiles_x tiles_y      -> eq_lut_offset eq_bytes
//   G ncols nrows pitch use            -> frame_geometry_refusal (use: a FrameUse value): the refusal's text, or "ok"
//   Q n  then n times "ncols nrows kind lean"  -> the groups of for_each_group, indices separated by blanks, groups by " | "
#include "ingest_rule.h"

#include <cstdio>
#include <vector>

using namespace kltapi;

struct Key { int nc, nr, kind, lean; };

int main()
{
    char q;
    while (std::scanf(" %c", &q) == 1) {
        if (q == 'E') {
            int nc, nr, tx, ty;
            if (std::scanf("%d %d %d %d", &nc, &nr, &tx, &ty) != 4) return 2;
            const char *why = equalisable_refusal(nc, nr, tx, ty);
            std::printf("%s\n", why ? why : "ok");
        } else if (q == 'S') {
            int nr, ty, batch;
            if (std::scanf("%d %d %d", &nr, &ty, &batch) != 3) return 2;
            std::printf("%d\n", eq_apply_split(nr, ty, batch));
        } else if (q == 'L') {
            int nc, nr, tx, ty;
            if (std::scanf("%d %d %d %d", &nc, &nr, &tx, &ty) != 4) return 2;
            std::printf("%zu %zu\n", eq_lut_offset(nc, nr), eq_bytes(nc, nr, tx, ty));
        } else if (q == 'G') {
            int nc, nr, pitch, use;
            if (std::scanf("%d %d %d %d", &nc, &nr, &pitch, &use) != 4) return 2;
            const char *why = frame_geometry_refusal(nc, nr, pitch, (FrameUse)use);
            std::printf("%s\n", why ? why : "ok");
        } else if (q == 'Q') {
            int n;
            if (std::scanf("%d", &n) != 1 || n < 0) return 2;
            std::vector<Key> keys((size_t)n);
            for (Key &k : keys)
                if (std::scanf("%d %d %d %d", &k.nc, &k.nr, &k.kind, &k.lean) != 4) return 2;
            std::vector<const Key *> items;
            for (const Key &k : keys) items.push_back(&k);
            bool first = true;
            const int rc = for_each_group(
                items.data(), items.size(),
                [](const Key *a, const Key *b) { return a->nc == b->nc && a->nr == b->nr && a->kind == b->kind && a->lean == b->lean; },
                [&](const Key *const *g, int count) {
                    if (count < 1 || count > KLT_MAX_BATCH) return 3;
                    if (!first) std::printf(" |");
                    first = false;
                    for (int b = 0; b < count; b++) std::printf(" %d", (int)(g[b] - keys.data()));
                    return 0;
                });
            if (rc) return rc;
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
