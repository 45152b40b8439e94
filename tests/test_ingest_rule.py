"""The host rules of the frame ingest path without a GPU: csrc/ingest_rule.h -- which frame geometry an entry point takes, which frame
the CLAHE stage equalises, how its buffer and its apply launch are laid out, how the slots of a call are gathered into launches -- is
compiled into tests/ingest_rule_dump.cpp, a stand-alone host program under the address and undefined-behaviour sanitizers, and asked;
the answers are held against the Python restatements the GPU tests use (params.equalisable, ingest_edges_expected.clahe_split and
.groups) and against the accept / refuse tables below."""
import os
import subprocess

import pytest

import ingest_edges_expected as ie

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPLOADED, ADOPTED, HOST = 0, 1, 2                            # FrameUse
# the answers of frame_geometry_refusal and equalisable_refusal: the library's refusal texts (KLT_ERR_ARG), "ok" for none
OK, BAD = "ok", "bad image geometry"
NOT_CONTIGUOUS = "an adopted frame must have contiguous rows (pitch == ncols): it is read in place"
TOO_LARGE = "frame too large (2^27 pixels or more: a plane of pixel records must stay below 2 GB)"
BELOW_GRID = "equalisation: the frame is smaller than the tile grid"
TILES_TOO_LARGE = "equalisation: tiles too large for a 32-bit interpolation (the largest Dx * Dy * 255 must stay below 2^32)"
MAX_PIXELS = 2 ** 27 - 1                                     # kMaxFramePixels


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ingest_rule") / "ingest_rule_dump")
    # host code only: a stand-alone program with its own main, the sanitizers' runtimes linked into it
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-Wno-cuda-compat",
                    "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "pyfeaturetrack_amd", "csrc"),
                    os.path.join(REPO, "tests", "ingest_rule_dump.cpp"), "-o", path], check=True)

    def ask(questions):
        """one answer line per question line"""
        r = subprocess.run([path], input="\n".join(questions) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, "ingest_rule_dump: exit %d\n%s" % (r.returncode, r.stderr[-2000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(questions), (len(lines), len(questions))
        return lines
    return ask


def test_equalisable(ask):
    from pyfeaturetrack_amd.params import equalisable
    cases = [(c.ncols, c.nrows, c.tiles_x, c.tiles_y) for c in ie.CLAHE_EDGES.values()] + list(ie.CLAHE_REFUSED)
    cases += [(nc, nr, tx, ty) for nc in (1, 2, 65535) for nr in (1, 2, 65535) for tx in (1, 2, 63, 64) for ty in (1, 2, 63, 64)]
    got = ask(["E %d %d %d %d" % case for case in cases])
    seen = set()
    for case, answer in zip(cases, got):
        nc, nr, tx, ty = case
        want = BELOW_GRID if tx > nc or ty > nr else (OK if equalisable(*case) else TILES_TOO_LARGE)
        assert answer == want and (want == OK) == equalisable(*case), (case, answer, want)
        seen.add(want)
    assert seen == {OK, BELOW_GRID, TILES_TOO_LARGE}
    assert all(not equalisable(*case) for case in ie.CLAHE_REFUSED)


def test_apply_split_and_lut_layout(ask):
    cases = [(nr, ty, batch) for nr in (1, 4, 8, 45, 1080, 65535) for ty in (1, 2, 8, 64) for batch in (1, 2, 32)]
    for case, answer in zip(cases, ask(["S %d %d %d" % case for case in cases])):
        assert int(answer) == ie.clahe_split(*case)[0], (case, answer)
    # the equalised frame rounded up to 256 bytes, then 256 bytes per tile
    sizes = [(1, 1), (255, 1), (256, 1), (257, 1), (67, 45)]
    assert [nc * nr for nc, nr in sizes] == [1, 255, 256, 257, 3015]
    tiles = [(1, 1), (3, 2), (64, 64)]
    cases = [(nc, nr, tx, ty) for nc, nr in sizes for tx, ty in tiles]
    for (nc, nr, tx, ty), answer in zip(cases, ask(["L %d %d %d %d" % case for case in cases])):
        offset, total = answer.split()
        want = -(-nc * nr // 256) * 256
        assert (int(offset), int(total)) == (want, want + 256 * tx * ty), (nc, nr, tx, ty, offset, total)
    assert -(-3015 // 256) * 256 == 3072 and -(-256 // 256) * 256 == 256 and -(-257 // 256) * 256 == 512


def test_frame_geometry(ask):
    """2^27 - 1 = 7 * 73 * 262657 has no factorisation with both sides in 1 .. 65535, so the largest frame there is has 2^27 - 2 pixels
    (2731 x 49146): that one is taken, 16384 x 8192 = 2^27 is not."""
    cases = []
    for use in (UPLOADED, ADOPTED, HOST):
        for side, want in ((0, BAD), (1, OK), (65535, OK), (65536, BAD)):
            cases += [((side, 1, side, use), want), ((1, side, 1, use), want)]
        too_large = BAD if use == HOST else TOO_LARGE        # (the host-frame calls answer one "bad image geometry")
        cases += [((2731, 49146, 2731, use), OK), ((16384, 8192, 16384, use), too_large), ((511, 262657, 511, use), BAD)]
    assert 2731 * 49146 == MAX_PIXELS - 1 and 16384 * 8192 == MAX_PIXELS + 1 and 511 * 262657 == MAX_PIXELS
    for use, short, wide in ((UPLOADED, BAD, OK), (ADOPTED, NOT_CONTIGUOUS, NOT_CONTIGUOUS), (HOST, BAD, OK)):
        cases += [((67, 45, 66, use), short), ((67, 45, 67, use), OK), ((67, 45, 68, use), wide)]
    # the host-frame form bounds the padded frame as well: pitch * nrows on either side of 2 * kMaxFramePixels, under frames that pass
    # every other test (pitch >= ncols, ncols * nrows <= 2^27 - 1); an upload of the same shape is taken
    assert 262657 * 1022 == 2 * MAX_PIXELS == 2 ** 28 - 2 and 65535 * 1022 <= MAX_PIXELS
    assert 14351 * 18705 == 2 ** 28 - 1 and 7000 * 18705 <= MAX_PIXELS
    cases += [((65535, 1022, 262657, HOST), OK), ((7000, 18705, 14351, HOST), BAD), ((7000, 18705, 14351, UPLOADED), OK)]
    got = ask(["G %d %d %d %d" % case for case, _ in cases])
    for (case, want), answer in zip(cases, got):
        assert answer == want, (case, answer, want)


BIG, SMALL = (67, 45, 1, 0), (40, 30, 1, 0)                  # (ncols, nrows, kind, lean)
GROUP_LISTS = {
    "empty": [],
    "one": [BIG],
    "32_equal": [BIG] * 32,
    "33_equal": [BIG] * 33,
    "65_equal": [BIG] * 65,
    "clahe_33_and_3_slots": [SMALL if k in (5, 17, 30) else BIG for k in range(36)],
    "alternating": [BIG, SMALL] * 20,
    "kind_differs": [BIG, (67, 45, 2, 0), BIG, (67, 45, 2, 0)],
    "lean_differs": [BIG, (67, 45, 1, 1), (67, 45, 1, 1), BIG],
}
GROUP_SIZES = {"empty": [], "one": [1], "32_equal": [32], "33_equal": [32, 1], "65_equal": [32, 32, 1], "clahe_33_and_3_slots": [32, 3, 1],
               "alternating": [20, 20], "kind_differs": [2, 2], "lean_differs": [2, 2]}


def test_grouping(ask):
    names = list(GROUP_LISTS)
    got = ask(["Q %d %s" % (len(GROUP_LISTS[n]), " ".join("%d %d %d %d" % k for k in GROUP_LISTS[n])) for n in names])
    for name, answer in zip(names, got):
        keys = GROUP_LISTS[name]
        found = [[int(w) for w in part.split()] for part in answer.split("|")] if answer.strip() else []
        assert found == ie.groups(keys), (name, found)
        assert [len(g) for g in found] == GROUP_SIZES[name], (name, found)
        assert sorted(i for g in found for i in g) == list(range(len(keys))), name       # every index exactly once
        for g in found:
            assert g == sorted(g) and len({keys[i] for i in g}) == 1 and len(g) <= ie.MAX_BATCH, (name, g)
        assert [g[0] for g in found] == sorted(g[0] for g in found), name                # first-appearance order
    assert ie.groups(GROUP_LISTS["clahe_33_and_3_slots"])[1] == [5, 17, 30]
