"""CPU test of matchmaker_amd/csrc/launch_geometry.h, the host arithmetic that decides which pairs a wavefront scores: the
header is compiled on its own by the system C++ compiler (tests/launch_geometry_check.cpp, no HIP) and its numbers are held
against the covering property of the wave split and against the Python mirrors of the all-pairs maps in test_host_cpu.py."""
import os
import shutil
import subprocess

import pytest

from tests import test_host_cpu as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256

# (n_pairs, maximum wavefronts): none, one, just below / at / just above the maximum, a remainder, and more than 2^31 pairs
MAXES = (1, 4, 1024, 2048, 4096)
SPLITS = [(n, m) for m in MAXES for n in (0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 1000003, (1 << 31) + 12345,
                                          (1 << 40) + 7) if n >= 0]


def _cases(test):
    (mark,) = [m for m in test.pytestmark if m.name == "parametrize"]
    assert mark.args[0] == "Bq,Bd,NQT"
    return list(mark.args[1])


TILED = _cases(H.test_tiled_all_pairs_work_map_covers_every_pair_once)
RING = _cases(H.test_shared_ring_all_pairs_work_map_covers_every_pair_once)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is part of the image"
    exe = str(tmp_path_factory.mktemp("geometry") / "launch_geometry_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "matchmaker_amd", "csrc"),
                    os.path.join(ROOT, "tests", "launch_geometry_check.cpp"), "-o", exe], check=True)

    def run(mode, rows):
        out = subprocess.run([exe, mode] + [str(x) for r in rows for x in r], check=True, capture_output=True, text=True).stdout
        lines = [l.split() for l in out.splitlines()]
        assert lines[0] == ["kCUs", str(CUS)]            # the mirrors' `cus`
        return [(l[0], *map(int, l[1:])) for l in lines[1:]]
    return run


def test_wave_split_covers_every_pair_once_with_no_idle_wavefront(check):
    got = check("split", SPLITS)
    assert [(n, m) for _, n, m, _, _ in got] == SPLITS
    for _, n, m, per, grid in got:
        assert per >= 1
        assert grid * per >= n, (n, m, per, grid)              # every pair has a wavefront
        assert (grid - 1) * per < n, (n, m, per, grid)         # ... and every wavefront a pair
        assert grid <= m, (n, m, per, grid)


def _mirror(Bq, Bd, q_per_group, target):
    """(gw, T, grid) as the mirrors in test_host_cpu.py compute them (their first four lines)."""
    G = (Bq + q_per_group - 1) // q_per_group
    gw = min(G, target)
    T = max(1, min(target // gw, (Bd + 7) // 8))
    return gw, T, 8 * T * gw


def test_all_pairs_maps_equal_the_python_mirrors(check):
    """The mirrors prove that a (gw, T) map covers every (query, document) pair once; this ties the launchers' arithmetic to
    them: both kernels' parameters on both mirrors' size lists."""
    cases = TILED + RING
    got = check("maps", cases)
    assert len(got) == 2 * len(cases)
    for i, (Bq, Bd, NQT) in enumerate(cases):
        tiled, ring = got[2 * i], got[2 * i + 1]
        assert tiled[:4] == ("tiled", Bq, Bd, NQT) and ring[:4] == ("ring", Bq, Bd, NQT)
        assert tiled[4:] == _mirror(Bq, Bd, NQT, CUS * 4 // 8), (Bq, Bd, NQT)
        assert ring[4:] == _mirror(Bq, Bd, 4 * NQT, CUS * 2 // 8), (Bq, Bd, NQT)


def test_all_pairs_maps_refuse_index_ranges_past_32_bits(check):
    """grid == 0 = "index range too large" (the launchers then fall back to one query per wavefront): the tiled kernel numbers a
    wavefront's (query group, document) items with 32 bits, the shared-ring kernel its documents."""
    big = 3_000_000_000
    rows = {(k, bq, bd): (gw, t, grid) for k, bq, bd, _, gw, t, grid in
            check("maps", [(big, big, 4), (4, (1 << 31) - 1, 4), (4, 1 << 31, 4), (1 << 20, 1 << 20, 4)])}
    assert rows[("tiled", big, big)][2] == 0 and rows[("ring", big, big)][2] == 0
    assert rows[("ring", 4, (1 << 31) - 1)][2] > 0 and rows[("ring", 4, 1 << 31)][2] == 0
    # one query group against 2^31 documents: 2^31 / 1024 slices' worth of items per wavefront still fits
    assert rows[("tiled", 4, 1 << 31)] == _mirror(4, 1 << 31, 4, CUS * 4 // 8)
    # 2^18 query groups / 128 lanes x (2^20 / 8 + 1) documents per wavefront = 2^28 + 2^11 items: fits; nothing is refused early
    assert rows[("tiled", 1 << 20, 1 << 20)] == _mirror(1 << 20, 1 << 20, 4, CUS * 4 // 8)
