// The host side of the descriptor and match rules (include/klt_gpu.h, "descriptors") that needs no device: the
// 256 tests of the pattern, generated and never typed in; the cosine table of the 32 orientation bins; and how many ranges the train
// set of a match is cut into.  Plain C++17 -- no HIP call in here; KLT_RULE_HD marks what a kernel calls too -- so that the rules are checked where there is no GPU
// (tests/test_describe_rule.py compiles this into tests/describe_rule_dump.cpp).  api_describe.hip sends the pattern to the device and
// launches from the answers; it decides nothing of this itself.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KLT_RULE_HD __host__ __device__
#else
#define KLT_RULE_HD
#endif

namespace kltapi {

constexpr int kDescTests = 256;           // bits of a descriptor
constexpr int kDescReach = 13;            // largest magnitude of a test coordinate, rotated or not
constexpr int kDescBox = 2;               // the box sums are (2 * 2 + 1)^2 pixels
constexpr int kDescDisc = 15;             // radius of the orientation disc = kDescReach + kDescBox: the patch is 31 x 31
constexpr int kDescBins = 32;             // orientation bins

// C[k] = round(16384 cos(2 pi k / 32)); S[k] = C[(k + 24) % 32]
constexpr int kDescCos[kDescBins] = {16384, 16069, 15137, 13623, 11585, 9102, 6270, 3196, 0, -3196, -6270, -9102, -11585, -13623, -15137, -16069,
                                     -16384, -16069, -15137, -13623, -11585, -9102, -6270, -3196, 0, 3196, 6270, 9102, 11585, 13623, 15137, 16069};
inline int desc_cos(int k) { return kDescCos[k & 31]; }
inline int desc_sin(int k) { return kDescCos[(k + 24) & 31]; }

// The pattern: tests[t] = (ax, ay, bx, by), all in -13 .. 13.  Draws of a 32-bit linear congruential generator, four per test; a
// test is discarded when a point lies outside the circle of radius 13, when its points coincide, or when it -- or its swap -- is in the
// list already.  Returns the number of draws consumed (1892).
inline int desc_pattern(int8_t tests[kDescTests][4])
{
    uint32_t s = 0x9E3779B9u;
    int draws = 0, n = 0;
    auto draw = [&]() {
        s = s * 1664525u + 1013904223u;
        draws++;
        return (int)((s >> 16) % 27u) - 13;
    };
    while (n < kDescTests) {
        const int ax = draw(), ay = draw(), bx = draw(), by = draw();
        if (ax * ax + ay * ay > 169 || bx * bx + by * by > 169 || (ax == bx && ay == by)) continue;
        bool seen = false;
        for (int i = 0; i < n && !seen; i++) {
            const int8_t *t = tests[i];
            seen = (t[0] == ax && t[1] == ay && t[2] == bx && t[3] == by) || (t[0] == bx && t[1] == by && t[2] == ax && t[3] == ay);
        }
        if (seen) continue;
        tests[n][0] = (int8_t)ax; tests[n][1] = (int8_t)ay; tests[n][2] = (int8_t)bx; tests[n][3] = (int8_t)by;
        n++;
    }
    return draws;
}

// ---- the match launch
constexpr int kMatchBlock = 64;           // queries of a workgroup, one per lane
constexpr int kMatchTile = 256;           // train records of a tile in LDS
constexpr int kMatchMaxSplits = 64;
constexpr int kMatchWorkgroups = 512;     // what a launch aims for: two workgroups per compute unit

// How many ranges the train set is cut into (blockIdx.y of the match launch), from (nq, nt) alone: enough that a short query list
// still fills the chip, no range shorter than a tile, at most kMatchMaxSplits.  klt_match_path reports it.
inline int match_splits(int nq, int nt)
{
    if (nq <= 0 || nt <= 0) return 1;
    const int blocks = (int)(((long long)nq + kMatchBlock - 1) / kMatchBlock);
    const int want = (kMatchWorkgroups + blocks - 1) / blocks;
    const int tiles = (int)(((long long)nt + kMatchTile - 1) / kMatchTile);
    int s = want < tiles ? want : tiles;
    if (s > kMatchMaxSplits) s = kMatchMaxSplits;
    return s < 1 ? 1 : s;
}
// the range of split `k` of `splits`: whole tiles, the first ranges one tile longer where they do not divide
KLT_RULE_HD inline void match_range(int nt, int splits, int k, int *lo, int *hi)
{
    const int tiles = (int)(((long long)nt + kMatchTile - 1) / kMatchTile);
    const int base = tiles / splits, extra = tiles % splits;
    const long long t0 = (long long)k * base + (k < extra ? k : extra), t1 = t0 + base + (k < extra ? 1 : 0);
    const long long a = t0 * kMatchTile, b = t1 * kMatchTile;
    *lo = (int)(a < nt ? a : nt);
    *hi = (int)(b < nt ? b : nt);
}

}  // namespace kltapi
