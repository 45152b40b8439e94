// The tracker's level-0 gradients on demand, on the host: the lane-independent arithmetic of the lazy tracker kernels
// (pyfeaturetrack_amd/csrc/track_primitives.h: lazy_row_h, lazy_col_v; klt_internal.h: corr_regs, reflect_once) applied to 14 x 14 patches
// cut from an image.  tests/test_lazy_grad_rule.py compiles this as host code under the address and undefined-behaviour sanitizers and holds
// the output against the oracle's gradient planes.  No kernel is launched and no GPU is needed.
//   lazy_grad_dump <in> <out>
//   in:  int32 ncols, nrows, n; double kg[4], kd[4] (the Gaussian and the derivative taps left of and at the centre); float image[nrows][ncols]
//        (the smoothed level-0 image); int32 corner[n][2] (cx, cy of an 8 x 8 footprint)
//   out: per footprint float gradx[8][8], grady[8][8]
// A footprint's patch is rows cy - 3 .. cy + 10, columns cx - 3 .. cx + 10 of the image through the reflect map, as the kernels cut it.  Each
// patch row goes through the row function once with eight outputs (the fused entry phase's form) and once per column with one output (the
// form of the phase per footprint), each footprint column through the column function likewise; the two forms must agree bit for bit, or
// the program fails.
#include <cstdio>
#include <cstring>
#include <vector>

#include "track_primitives.h"

static bool read_all(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int hdr[3];
    TapRegs<7> kg = {}, kd = {};
    if (!read_all(in, hdr, sizeof hdr) || !read_all(in, kg.k, 4 * sizeof(double)) || !read_all(in, kd.k, 4 * sizeof(double))) return 2;
    const int nc = hdr[0], nr = hdr[1], n = hdr[2];
    if (nc < 14 || nr < 14 || nc > 65535 || nr > 65535 || n < 0 || n > 1 << 20) return 2;
    std::vector<float> img((size_t)nc * nr);
    std::vector<int> corner(2 * (size_t)n);
    if (!read_all(in, img.data(), img.size() * sizeof(float)) || !read_all(in, corner.data(), corner.size() * sizeof(int))) return 2;
    fclose(in);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int f = 0; f < n; f++) {
        const int cx = corner[2 * f], cy = corner[2 * f + 1];
        if (cx - 3 < -nc || cx + 10 >= 2 * nc || cy - 3 < -nr || cy + 10 >= 2 * nr) return 3;      // what reflect_once maps
        float patch[14][14], d[14][8], e[14][8];
        for (int r = 0; r < 14; r++)
            for (int c = 0; c < 14; c++) patch[r][c] = img[(size_t)reflect_once(cy - 3 + r, nr) * nc + reflect_once(cx - 3 + c, nc)];
        for (int r = 0; r < 14; r++) {
            lazy_row_h<8>(patch[r], kg, kd, d[r], e[r]);
            for (int c = 0; c < 8; c++) {
                float d1, e1;
                lazy_row_h<1>(patch[r] + c, kg, kd, &d1, &e1);
                if (memcmp(&d1, &d[r][c], 4) || memcmp(&e1, &e[r][c], 4)) {
                    fprintf(stderr, "footprint %d, patch row %d, column %d: the row function's two forms differ\n", f, r, c);
                    return 4;
                }
            }
        }
        float g[2][8][8];
        for (int c = 0; c < 8; c++) {
            float cd[14], ce[14], gx[8], gy[8];
            for (int r = 0; r < 14; r++) { cd[r] = d[r][c]; ce[r] = e[r][c]; }
            lazy_col_v<1, 8>(cd, kg, gx);
            lazy_col_v<-1, 8>(ce, kd, gy);
            for (int r = 0; r < 8; r++) {
                float x1, y1;
                lazy_col_v<1, 1>(cd + r, kg, &x1);
                lazy_col_v<-1, 1>(ce + r, kd, &y1);
                if (memcmp(&x1, &gx[r], 4) || memcmp(&y1, &gy[r], 4)) {
                    fprintf(stderr, "footprint %d, row %d, column %d: the column function's two forms differ\n", f, r, c);
                    return 4;
                }
                g[0][r][c] = gx[r];
                g[1][r][c] = gy[r];
            }
        }
        if (fwrite(g, sizeof g, 1, out) != 1) return 2;
    }
    return fclose(out) ? 2 : 0;
}
