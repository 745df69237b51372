"""Generates tests/golden/abi4_signatures.json: the prototypes of ABI 4 as the ctypes binding holds them,
{symbol: [return type, [argument type, ...]]} in the names int, int64, size_t, float, double, ptr, str.

The committed file was written at the last commit whose matchmaker_amd/_lib.py spelled SIGNATURES out by hand, so it is
independent of the reader that now derives the table from include/mm_native.h; tests/test_abi_cpu.py holds the derived
table to it.  It freezes ABI 4: symbols added later need no entry, and a frozen prototype changes only together with
MM_ABI_VERSION, which is when to run this again (python tests/golden/gen_golden_abi.py, into a file named for the new version).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "abi4_signatures.json")

NAMES = {ctypes.c_int: "int", ctypes.c_int64: "int64", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
         ctypes.c_double: "double", ctypes.c_void_p: "ptr", ctypes.c_char_p: "str"}


def dump(signatures):
    """{symbol: (restype, [argtypes])} of ctypes classes -> the JSON text, one symbol per line, in table order"""
    rows = [f' "{name}": ' + json.dumps([NAMES[res], [NAMES[a] for a in args]]) for name, (res, args) in signatures.items()]
    return "{\n" + ",\n".join(rows) + "\n}\n"


def main():
    from matchmaker_amd import _lib
    with open(OUT, "w") as f:
        f.write(dump(_lib.SIGNATURES))
    print(OUT, len(_lib.SIGNATURES), "symbols")


if __name__ == "__main__":
    main()
