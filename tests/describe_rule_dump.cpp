// TEST INFRASTRUCTURE ONLY -- the host side of the descriptor and match rules (csrc/describe_rule.h) answered one question per input line,
// for tests/test_describe_rule.py.  A stand-alone host program: built under the address and undefined-behaviour sanitizers, never loaded
// into anything.  Questions on stdin, answers on stdout, one line each:
//   P          -> the draws consumed, then the 256 tests as 1024 integers
//   C          -> the 32 cosines, then the 32 sines
//   S nq nt    -> match_splits, then the ranges of match_range as "lo hi" pairs
#include "describe_rule.h"

#include <cstdio>

using namespace kltapi;

int main()
{
    char q;
    while (std::scanf(" %c", &q) == 1) {
        if (q == 'P') {
            int8_t tests[kDescTests][4];
            std::printf("%d", desc_pattern(tests));
            for (int t = 0; t < kDescTests; t++)
                for (int k = 0; k < 4; k++) std::printf(" %d", (int)tests[t][k]);
            std::printf("\n");
        } else if (q == 'C') {
            for (int k = 0; k < kDescBins; k++) std::printf("%d ", desc_cos(k));
            for (int k = 0; k < kDescBins; k++) std::printf("%d%s", desc_sin(k), k + 1 < kDescBins ? " " : "\n");
        } else if (q == 'S') {
            int nq, nt;
            if (std::scanf("%d %d", &nq, &nt) != 2) return 2;
            const int splits = match_splits(nq, nt);
            std::printf("%d", splits);
            for (int k = 0; k < splits; k++) {
                int lo, hi;
                match_range(nt, splits, k, &lo, &hi);
                std::printf(" %d %d", lo, hi);
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
