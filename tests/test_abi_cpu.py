"""CPU tests of the binding itself: matchmaker_amd/_lib.py derives its table of prototypes and its constants from
include/mm_native.h, and this module holds the derivation to a picture of ABI 4 taken from the last hand-written table
(tests/golden/abi4_signatures.json, tests/golden/gen_golden_abi.py).  The same file is the project's ABI guard: a frozen
prototype that changes or disappears without a new MM_ABI_VERSION fails here; symbols added since need no entry."""
import ctypes
import json
import os
import re

import pytest

from matchmaker_amd import _lib
from matchmaker_amd._lib import NativeError
from tests import abi, util

CTYPES = {"int": ctypes.c_int, "int64": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
          "double": ctypes.c_double, "ptr": ctypes.c_void_p, "str": ctypes.c_char_p}


def test_derived_signatures_match_the_frozen_picture_of_abi_4():
    with open(os.path.join(util.GOLDEN, "abi4_signatures.json")) as f:
        frozen = json.load(f)
    assert len(frozen) == 73
    for name, (ret, args) in frozen.items():
        assert name in _lib.SIGNATURES, f"{name} is part of ABI 4 and is no longer declared"
        res, argtypes = _lib.SIGNATURES[name]
        assert res is CTYPES[ret], (name, "return", ret, res)
        assert len(argtypes) == len(args), (name, len(args), len(argtypes))
        for i, (want, got) in enumerate(zip(args, argtypes)):
            assert got is CTYPES[want], f"{name}: argument {i} is frozen as {want}, the header now gives {got.__name__}"
    # nothing the header declares escapes the reader: a plain scan for `mm_name (` over the prototypes finds the same set
    prototypes = re.sub(r"^[ \t]*#.*$", "", abi.header_code(), flags=re.M)
    assert set(re.findall(r"\b(mm_\w+)\s*\(", prototypes)) == set(_lib.SIGNATURES)


def test_derived_constants_are_the_values_the_hand_written_binding_had():
    want = dict(MM_F32=0, MM_F16=1, MM_BF16=2, MASK_NONE=0, MASK_LEN_I32=1, MASK_U8=2, MASK_I64=3, MASK_F32=4,
                TKL_SAT_EMBEDDING=0, TKL_SAT_LOG=1, SIM_ROUND=1, SUM_ROUND=2, STORE_KEEP_ZERO_ROWS=1, ABI_VERSION=4,
                MM_OK=0, MM_EINVAL=-1, MM_EUNSUPPORTED=-2, MM_EWORKSPACE=-3, MM_ELAUNCH=-4,
                RANK_MAX_LEN=8192, RANK_MAX_CUTOFFS=8, RANK_NOT_JUDGED=-2 ** 31)
    got = {name: getattr(_lib, name) for name in want}
    assert got == want and all(type(v) is int for v in got.values())
    from matchmaker_amd import build
    build.build()
    assert _lib.ABI_VERSION == 4 == _lib.lib().mm_abi_version()


@pytest.mark.parametrize("text,offender", [
    ("int mm_f(long n);", "long n"), ("int mm_f(int a, unsigned b);", "unsigned b"), ("int mm_f(unsigned int b);", "unsigned int b"),
    ("int mm_f(mm_maxsim_batch_t b);", "mm_maxsim_batch_t b"), ("int mm_f(struct s b);", "struct s b"), ("int mm_f(int a[4]);", "int a[4]"),
    ("long mm_f(int a);", "long"), ("void mm_f(int a);", "void"), ("const void* mm_f(void);", "const void*"),
    ("unsigned int mm_f(void);", "unsigned int")])
def test_reader_refuses_what_it_cannot_bind_and_names_the_symbol(text, offender):
    with pytest.raises(NativeError) as e:
        _lib._read_header("int mm_ok(void);\n" + text + "\n")
    assert "mm_f" in str(e.value) and repr(offender) in str(e.value) and "mm_ok" not in str(e.value)
    with pytest.raises(NativeError, match="MM_NAME"):
        _lib._read_header('#define MM_NAME "text"\n')


def test_reader_skips_comments_macros_and_struct_typedefs():
    sigs, defines = _lib._read_header("""
/* int mm_in_a_block_comment(int a);
 * see mm_prose() */
// int mm_in_a_line_comment(long a);
#ifndef MM_GUARD
#define MM_GUARD
#define MM_TWO 2 /* a comment that
                    runs on */
#define MM_NEG (-2147483647 - 1)   // INT32_MIN
#define MM_MACRO(K, E) (4 * (K) + mm_in_a_macro(E))
typedef struct {
  const void* q;
  int64_t n;
} mm_thing_t;
int mm_abi_version(void);
const char *mm_last_error( void );
size_t mm_sizes(int64_t n, size_t bytes,
                float x, double y, int);
int mm_pointers(const mm_thing_t* t, const void* const* list, float* out, const int64_t *rows, void* stream);
#endif
""")
    c = ctypes
    assert sigs == {"mm_abi_version": (c.c_int, []), "mm_last_error": (c.c_char_p, []),
                    "mm_sizes": (c.c_size_t, [c.c_int64, c.c_size_t, c.c_float, c.c_double, c.c_int]),
                    "mm_pointers": (c.c_int, [c.c_void_p] * 5)}
    assert list(sigs) == ["mm_abi_version", "mm_last_error", "mm_sizes", "mm_pointers"]      # header order
    assert defines == {"MM_TWO": 2, "MM_NEG": -2 ** 31}


def test_every_derived_symbol_is_exported_and_size_queries_need_no_gpu():
    L = abi.assert_bound(tuple(_lib.SIGNATURES))
    # size queries are pure host arithmetic: callable without a GPU
    assert L.mm_maxsim_workspace_bytes(10, 1, 32, 180, _lib.MASK_NONE, _lib.MASK_LEN_I32) == 0
    assert L.mm_maxsim_workspace_bytes(10, 1, 32, 180, _lib.MASK_I64, _lib.MASK_I64) > 0
