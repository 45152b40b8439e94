"""The lazy tracker's level-0 gradients without a GPU: the lane-independent arithmetic of both kernel forms (track_primitives.h: lazy_row_h,
lazy_col_v over corr_regs; reflect_once) is compiled as host code into tests/lazy_grad_dump.cpp, under the address and undefined-behaviour
sanitizers, and applied to 14 x 14 patches of the oracle's smoothed level-0 image of tests/golden/img0.pgm.  What comes out must be the
oracle's own gradx / grady planes at the 8 x 8 footprints, bit for bit: the tracker on a lean slot computes exactly these values in
place of reading them from the level's records.

About 200 footprints: a seeded draw over the whole image, plus footprints whose patch leaves the image on each of the four sides and at
the four corners by one, two and three pixels (the footprint itself stays inside, or there would be no plane to compare with), where
the patch is cut through the reflect map."""
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import make_tc, params_from_tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corners(nc, nr):
    rng = np.random.default_rng([14, 14])
    cs = [(int(x), int(y)) for x, y in zip(rng.integers(0, nc - 7, 160), rng.integers(0, nr - 7, 160))]
    mid_x, mid_y = nc // 2 - 4, nr // 2 - 4
    for e in (0, 1, 2):                                  # the patch leaves the image by 3 - e pixels
        lo, hx, hy = e, nc - 8 - e, nr - 8 - e
        cs += [(lo, mid_y + e), (hx, mid_y - e), (mid_x + e, lo), (mid_x - e, hy), (lo, lo), (hx, lo), (lo, hy), (hx, hy)]
    cs += [(3, 3), (nc - 11, nr - 11), (2, nr - 11), (nc - 11, 2)]          # the patch ends at the image's edge, and one short of it
    return cs


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lazy_grad") / "lazy_grad_dump")
    # host code only: a stand-alone program with its own main, the sanitizers' runtimes linked into it
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function",
                    "-Wno-cuda-compat", "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "pyfeaturetrack_amd", "csrc"),
                    os.path.join(REPO, "tests", "lazy_grad_dump.cpp"), "-o", path], check=True)
    return path


def test_host_gradients_are_the_oracles_planes(exe, img0, tmp_path):
    from oracle import klt_oracle as ko
    from pyfeaturetrack_amd.params import taps_from_params
    p = params_from_tc(make_tc(levels=3, ss=4))
    pyr = ko.Pyramids(p, img0.astype(np.float32))
    img, gx, gy = (pyr.level(k, 0) for k in ("img", "gx", "gy"))
    nr, nc = img.shape
    gauss, deriv = taps_from_params(p)[2]
    assert len(gauss) == 7 and len(deriv) == 7, "the lazy tracker exists for 7-tap gradient filters"
    cs = _corners(nc, nr)
    assert len(cs) >= 180
    reflected = [c for c in cs if c[0] < 3 or c[1] < 3 or c[0] + 10 >= nc or c[1] + 10 >= nr]
    assert len(reflected) >= 24
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", nc, nr, len(cs)))
        # the taps as the library keeps them (klt_set_kernels: reversed, as scipy's convolve1d hands them to correlate1d); the kernels
        # carry the four left of and at the centre
        f.write(np.asarray(gauss[::-1][:4], np.float64).tobytes())
        f.write(np.asarray(deriv[::-1][:4], np.float64).tobytes())
        f.write(np.ascontiguousarray(img, np.float32).tobytes())
        f.write(np.asarray(cs, np.int32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, "lazy_grad_dump: exit %d\n%s" % (r.returncode, r.stderr[-2000:])
    got = np.fromfile(fout, np.float32).reshape(len(cs), 2, 8, 8)
    for i, (cx, cy) in enumerate(cs):
        for k, (name, plane) in enumerate((("gradx", gx), ("grady", gy))):
            want = plane[cy:cy + 8, cx:cx + 8]
            assert got[i, k].tobytes() == np.ascontiguousarray(want).tobytes(), \
                "footprint at (%d, %d): %s differs from the oracle's plane, max |d| = %g" % (cx, cy, name, np.abs(got[i, k] - want).max())
