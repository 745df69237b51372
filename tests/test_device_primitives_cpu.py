"""CPU test of the host-callable device primitives: the order-preserving sort keys and pow2_ge of
matchmaker_amd/csrc/bitonic_device.h and the bf16 rounding of elem_device.h.  The headers are compiled on their own by the
system C++ compiler (tests/device_primitives_check.cpp, no HIP) - a second time with the address / undefined-behaviour
sanitizers where their runtimes are installed - and the numbers are held against the order of the floats, against the
inverses, and for the rounding against torch's float32 -> bfloat16 conversion on the CPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ascending: -inf, -FLT_MAX, -1, -smallest normal, -largest denormal, -smallest denormal, -0,
#            +0, smallest denormal, largest denormal, smallest normal, 1, the next float after 1, FLT_MAX, +inf
ORDERED = [0xff800000, 0xff7fffff, 0xbf800000, 0x80800000, 0x807fffff, 0x80000001, 0x80000000,
           0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x3f800001, 0x7f7fffff, 0x7f800000]
NEG0, POS0 = 0x80000000, 0x00000000
NANS = [0x7fc00000, 0x7f800001, 0xffc00000, 0xff800001, 0x7fffffff, 0xffffffff]      # quiet, signalling, negative, all ones


def _compile(cxx, exe, extra=()):
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "matchmaker_amd", "csrc"),
                           os.path.join(ROOT, "tests", "device_primitives_check.cpp"), "-o", exe], capture_output=True, text=True)


SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(mode, words) -> the program's lines as tuples of ints.  The program is built twice where the compiler's sanitizer
    runtimes are installed (a plain executable with its own main), and then every run goes through both builds."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is part of the image"
    tmp = tmp_path_factory.mktemp("primitives")
    exes = [str(tmp / "device_primitives_check")]
    built = _compile(cxx, exes[0])
    assert built.returncode == 0, built.stderr
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode == 0:
        exes.append(str(tmp / "device_primitives_check_san"))
        built = _compile(cxx, exes[1], SANITIZE)
        assert built.returncode == 0, built.stderr

    def run(mode, words, base=16):
        outs = []
        for exe in exes:
            done = subprocess.run([exe, mode] + [str(w) for w in words], capture_output=True, text=True)
            assert done.returncode == 0, (exe, done.returncode, done.stderr)
            outs.append(done.stdout)
        assert all(o == outs[0] for o in outs)
        lines = [l.split() for l in outs[0].splitlines()]
        assert all(l[0] == mode for l in lines)
        return [tuple(int(x, base) for x in l[1:]) for l in lines]
    return run


def _hex(words):
    return [f"{w:08x}" for w in words]


@pytest.fixture(scope="module")
def keys(check):
    got = check("keys", _hex(ORDERED))
    assert [g[0] for g in got] == ORDERED
    return got


def test_descending_key_falls_along_the_floats_and_counts_minus_zero_as_plus_zero(keys):
    desc = {x: d for x, d, *_ in keys}
    for lo, hi in zip(ORDERED, ORDERED[1:]):
        if (lo, hi) == (NEG0, POS0):
            assert desc[lo] == desc[hi]
        else:
            assert desc[lo] > desc[hi], (hex(lo), hex(hi))
    for x, _, back, *_ in keys:
        assert back == (POS0 if x == NEG0 else x), hex(x)


def test_ascending_key_rises_along_the_floats_with_minus_zero_below_plus_zero(keys):
    asc = [a for _, _, _, a, _, _ in keys]
    assert all(lo < hi for lo, hi in zip(asc, asc[1:]))
    for x, _, _, _, back, _ in keys:
        assert back == x, hex(x)


def test_nan_rule_puts_every_nan_on_the_one_key_behind_minus_inf(check, keys):
    for x, d, _, _, _, nan_last in keys:
        assert nan_last == d, hex(x)                       # not a NaN: the descending key itself
    assert all(d < 0xffffffff for _, d, *_ in keys)        # ... and -inf's (the largest) is still in front of the NaNs'
    got = check("keys", _hex(NANS))
    assert [g[0] for g in got] == NANS
    assert all(g[5] == 0xffffffff for g in got)


def _finite_patterns():
    u = np.random.RandomState(20240607).randint(0, 1 << 32, size=600, dtype=np.uint64).astype(np.uint32)
    u = u[((u >> 23) & 0xff) != 0xff][:400]
    assert len(u) == 400
    return [int(x) for x in u]


# a tie to even and a tie to odd, just below / above a tie, the largest finite values' tie (rounds to inf), denormals, -0, +-inf
BF16_EDGES = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001, 0x7f7f8000, 0x7f7f7fff, 0xff7f8000,
              0x00000001, 0x00007fff, 0x00008000, 0x00008001, 0x007fffff, 0x80000001, 0x80000000, 0x00000000, 0x7f800000, 0xff800000]


def _torch_bf16_bits(words):
    f = torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32)).view(torch.float32)
    return [int(x) & 0xffff for x in f.to(torch.bfloat16).view(torch.int16).tolist()]


def test_bf16_rounding_equals_torch_on_edges_and_random_finite_patterns(check):
    words = BF16_EDGES + _finite_patterns()
    got = check("bf16", _hex(words))
    assert [g[0] for g in got] == words
    want = _torch_bf16_bits(words)
    assert dict(zip(BF16_EDGES, want))[0x3f808000] == 0x3f80 and dict(zip(BF16_EDGES, want))[0x3f818000] == 0x3f82
    assert dict(zip(BF16_EDGES, want))[0x7f7f8000] == 0x7f80
    for (x, rne, guarded), w in zip(got, want):
        assert rne == w, (hex(x), hex(rne), hex(w))
        assert guarded == w, (hex(x), hex(guarded), hex(w))      # the guard changes nothing but NaNs


def test_bf16_nan_guard_gives_the_quiet_nan(check):
    got = check("bf16", _hex(NANS))
    assert [g[0] for g in got] == NANS
    assert all(g[2] == 0x7fc0 for g in got)


def test_pow2_ge_is_exact_around_every_power_of_two(check):
    """int up to 2^30 (2^30 + 1 has no answer in an int: that one goes through the int64 overload), int64 up to 2^40."""
    cases = [(32, 0, 1), (32, 1, 1), (64, 0, 1), (64, 1, 1), (32, -5, 1), (64, -5, 1)]
    for k in range(1, 41):
        p = 1 << k
        below = p if k > 1 else 1                         # 2^1 - 1 = 1 -> 1
        for width in (32, 64):
            if width == 32 and k > 30:
                continue
            cases += [(width, p, p), (width, p - 1, below)]
            if not (width == 32 and k == 30):
                cases.append((width, p + 1, 2 * p))
    got = check("pow2", [x for w, v, _ in cases for x in (w, v)], base=10)
    assert got == cases
