// The rules of the frame ingest path that need no device: which frame geometry an entry point takes, which frame the CLAHE stage can
// equalise and how its buffer and its apply launch are laid out, and how the slots of a call are gathered into launches.  Plain C++17 -- no
// HIP in here -- so that the rules are checked where there is no GPU (tests/test_ingest_rule.py).  api_frames.hip turns the answers into
// return codes and decides nothing of this itself.
#pragma once
#include <algorithm>
#include <vector>

#include "l0_plan.h"      // KLT_MAX_BATCH

namespace kltapi {

// The kernels address a plane with 32-bit BYTE offsets into a buffer descriptor of 2 GB (raw buffer operations, klt_internal.h), and the
// largest plane is the record plane of level 0 with 12 bytes per pixel: a frame must stay below 2^27 pixels (1.5 GB of records).
// 16 384 x 8 191 pixels is such a frame, 16 384 x 8 192 is not; the largest frame of the test suite is 7680 x 4320.
constexpr long long kMaxFramePixels = (1LL << 27) - 1;
constexpr int kMaxFrameSide = 65535;

// ---- frame geometry
// Who brings the frame: an upload into a slot (rows `pitch` pixels apart), an adoption (read in place, so its rows must be contiguous), or
// a host frame that goes through one stage and comes back (klt_equalize_u8, klt_remap_u8: staged at its pitch, so the padded frame is
// bounded too -- by twice the pixel bound -- and every refusal is the one "bad image geometry").  The answer: why the frame is refused
// (KLT_ERR_ARG with this text), or null
enum FrameUse { FRAME_UPLOADED, FRAME_ADOPTED, FRAME_HOST };

inline const char *frame_geometry_refusal(int ncols, int nrows, int pitch, FrameUse use)
{
    const char *const bad = "bad image geometry";
    if (ncols < 1 || nrows < 1 || ncols > kMaxFrameSide || nrows > kMaxFrameSide) return bad;
    if (use == FRAME_ADOPTED && pitch != ncols) return "an adopted frame must have contiguous rows (pitch == ncols): it is read in place";
    if (pitch < ncols || (use == FRAME_HOST && (long long)pitch * nrows > 2 * kMaxFramePixels)) return bad;
    if ((long long)ncols * nrows <= kMaxFramePixels) return nullptr;
    return use == FRAME_HOST ? bad : "frame too large (2^27 pixels or more: a plane of pixel records must stay below 2 GB)";
}

// ---- CLAHE ingest stage (the rule: include/klt_gpu.h)
// A frame is equalisable when the tile grid fits it and the per-pixel division is a 32-bit one: the largest Dx * Dy * 255 below 2^32,
// Dx the largest distance of two neighbouring tile centres in doubled coordinates (1 with one tile on the axis)
inline long long widest_centre_gap(int n, int tiles)
{
    long long widest = 1;
    for (int k = 0; k + 2 <= tiles; k++)           // C_{k+1} - C_k = x_{k+2} - x_k
        widest = std::max(widest, ((long long)(k + 2) * n) / tiles - ((long long)k * n) / tiles);
    return widest;
}

// why a frame is not (KLT_ERR_ARG with this text), or null
inline const char *equalisable_refusal(int nc, int nr, int tiles_x, int tiles_y)
{
    if (tiles_x > nc || tiles_y > nr) return "equalisation: the frame is smaller than the tile grid";
    if (widest_centre_gap(nc, tiles_x) * widest_centre_gap(nr, tiles_y) * 255 >= (1LL << 32))
        return "equalisation: tiles too large for a 32-bit interpolation (the largest Dx * Dy * 255 must stay below 2^32)";
    return nullptr;
}

// the bytes of an equalised frame with its LUTs, and where the LUTs begin behind the frame
inline size_t eq_lut_offset(int nc, int nr) { return ((size_t)nc * nr + 255) & ~(size_t)255; }
inline size_t eq_bytes(int nc, int nr, int tiles_x, int tiles_y) { return eq_lut_offset(nc, nr) + (size_t)tiles_x * tiles_y * 256; }

// the apply launch on `batch` frames: every band of rows between two tile centres split until about a thousand workgroups are out, a
// workgroup keeping at least 4 rows of a band of average height
inline int eq_apply_split(int nrows, int tiles_y, int batch)
{
    const int bands = tiles_y + 1;
    const int split = (1024 + bands * batch - 1) / (bands * batch);
    const int most = std::max(1, nrows / tiles_y / 4);
    return std::max(1, std::min(split, most));
}

// ---- grouping
// The members of one call's list that share a launch: `items` walked in first-appearance order, body(group, count) called with up to
// KLT_MAX_BATCH members that same(first, member) calls equal -- a 33rd equal member opens a group of its own where it stands.  Every member
// goes out exactly once.  The first non-zero answer of `body` ends the walk and is returned.  (One heap block: the marks.)
template <class T, class Same, class Body>
int for_each_group(const T *items, size_t n, Same same, Body body)
{
    std::vector<bool> done(n, false);
    for (size_t i0 = 0; i0 < n; i0++) {
        if (done[i0]) continue;
        T group[KLT_MAX_BATCH];
        int count = 0;
        for (size_t i = i0; i < n && count < KLT_MAX_BATCH; i++)
            if (!done[i] && same(items[i0], items[i])) {
                group[count++] = items[i];
                done[i] = true;
            }
        if (int rc = body((const T *)group, count)) return rc;
    }
    return 0;
}

}  // namespace kltapi
