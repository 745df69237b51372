"""What every operator's CPU test asks of the C boundary, in one place (a helper, not a test module): that its entry points
are declared in include/mm_native.h, bound by matchmaker_amd/_lib.py and exported by the built library, and that a plain C
program can call them.  The prototypes' types are pinned by tests/test_abi_cpu.py against tests/golden/abi4_signatures.json."""
import functools
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def header_code():
    """include/mm_native.h without its comments (their prose names entry points, parentheses included)"""
    with open(os.path.join(INCLUDE, "mm_native.h")) as f:
        return re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def _built():
    from matchmaker_amd import build, _lib
    so = build.build()
    return so, _lib.lib(), header_code()           # lib() binds every symbol of SIGNATURES: AttributeError if one is missing


def assert_bound(names):
    """each name is declared in the header, present in _lib.SIGNATURES and exported by the built library, which is returned"""
    from matchmaker_amd import _lib
    _, L, code = _built()
    assert names, "no symbols named"
    for name in names:
        assert re.search(r"\b" + re.escape(name) + r"\s*\(", code), f"{name} is not declared in include/mm_native.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert hasattr(L, name), f"{name} is not exported by {_lib.LIB_PATH}"
    return L


def run_c_client(tmp_path, source, name="client"):
    """Compiles `source` as strict C99 against the header, links the built libmm_native.so, runs it; returns its stdout."""
    so = _built()[0]
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    src, exe, libdir = tmp_path / (name + ".c"), tmp_path / name, os.path.dirname(so)
    src.write_text(source)
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, str(src), "-o", str(exe),
                        "-L", libdir, "-l:libmm_native.so", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return r.stdout
