"""CPU test of matchmaker_amd/csrc/launch_geometry.h, the host arithmetic that decides which pairs a wavefront scores: the
header is compiled on its own by the system C++ compiler (tests/launch_geometry_check.cpp, no HIP) and its numbers are held
against the covering property of the wave split, against the Python mirrors of the all-pairs maps in test_host_cpu.py and,
for the workspace cursor, against the layout it is given: measured size = carved size, 256-byte blocks that do not overlap."""
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


def _compile(cxx, exe, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "matchmaker_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_geometry_check.cpp"), "-o", exe], capture_output=True, text=True)


SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(mode, rows) -> the program's lines.  The program is built twice where the compiler's address / undefined-behaviour
    sanitizer runtimes are installed (a plain executable with its own main), and then every run goes through both builds."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is part of the image"
    tmp = tmp_path_factory.mktemp("geometry")
    exes = [str(tmp / "launch_geometry_check")]
    built = _compile(cxx, exes[0])
    assert built.returncode == 0, built.stderr
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode == 0:
        exes.append(str(tmp / "launch_geometry_check_san"))
        built = _compile(cxx, exes[1], SANITIZE)
        assert built.returncode == 0, built.stderr

    def run(mode, rows):
        outs = []
        for exe in exes:
            done = subprocess.run([exe, mode] + [str(x) for r in rows for x in r], capture_output=True, text=True)
            assert done.returncode == 0, (exe, done.returncode, done.stderr)
            outs.append(done.stdout)
        assert all(o == outs[0] for o in outs)
        lines = [l.split() for l in outs[0].splitlines()]
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


def _a256(b):
    return (b + 255) // 256 * 256


# (count, element size) blocks of one layout: empty and one-element blocks, byte counts around and far from the multiples of 256,
# element sizes that divide 256 and that do not, the shapes of the IVF layout (ten blocks) and a single block
LAYOUTS = [
    [(1, 4)],
    [(0, 4)],
    [(0, 1), (0, 8), (0, 12)],
    [(0, 4), (1, 1), (0, 8), (1, 12), (1, 3)],
    [(255, 1), (256, 1), (257, 1), (1, 8), (63, 4), (64, 4), (65, 4)],
    [(85, 3), (86, 3), (21, 12), (22, 12), (1000003, 1), (7, 2)],
    [(6, 4), (6, 4), (3, 4), (4, 8), (2, 4), (5, 4), (5, 4), (6, 4), (8, 4), (120, 4)],
    [(3 * 16384, 4), (3, 4), (3, 4), (3 * 4096, 4), (3 * 4096, 4)],
]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "-".join(f"{c}x{s}" for c, s in l))
def test_cursor_measures_what_it_carves(check, layout):
    """A cursor without a base returns only null and ends at the size; the same takes on a buffer of exactly that size give
    256-byte aligned blocks, each as long as asked for, in order, none overlapping, all inside the buffer (the program also
    writes every block end to end, which the sanitizer build checks)."""
    *takes, total = check("cursor", layout)
    assert [(c, s) for _, c, s, *_ in takes] == layout
    end = 0
    for _, count, size, measured, carved, offset, null in takes:
        assert null == 1                                  # the measuring cursor formed no pointer
        assert offset % 256 == 0 and offset == end, (count, size, offset, end)      # aligned, and not before the previous block's end
        end = offset + _a256(count * size)
        assert offset + count * size <= end
        assert measured == carved == end, (count, size, measured, carved, end)
    assert total == ("total", end, end, 0)                # measured = consumed; nothing left of a buffer of that size

