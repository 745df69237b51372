"""ctypes binding of libmm_native.so.  include/mm_native.h is the one description of the C ABI: the table of prototypes and the
constants below are read from it at import, nothing is restated here.

There is NO fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
# MM_NATIVE_LIB: another build of the same library for ONE process (A/B variants, tools/build_variant.sh)
LIB_PATH = os.environ.get("MM_NATIVE_LIB") or os.path.join(HERE, "csrc", "libmm_native.so")
HEADER_PATH = os.path.join(HERE, "..", "include", "mm_native.h")


class NativeError(RuntimeError):
    """.code: the C return code (MM_E*) when the error came from libmm_native.so or restates one of its checks, else None."""

    def __init__(self, msg="", code=None):
        super().__init__(msg)
        self.code = code


_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}


def _read_header(text):
    """The text of a C header -> ({symbol: (restype, [argtypes])} of every prototype `RET mm_name(ARGS);`,
    {NAME: int} of every object-like #define with a value).  The header's vocabulary is small: three return types, five scalars,
    and every declarator with a `*` is a pointer.  Anything outside it is a NativeError naming the symbol, never a guess."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)$", text, re.M):   # NAME( is a macro: no match
        terms = re.sub(r"\s", "", value)                                     # a decimal integer or a sum of them: (-2147483647 - 1)
        if not re.fullmatch(r"\(?[-+]?(0|[1-9]\d*)([-+](0|[1-9]\d*))*\)?", terms):
            raise NativeError(f"#define {name}: cannot read the value {value.strip()!r}")
        defines[name] = sum(int(t) for t in re.findall(r"[-+]?\d+", terms))
    signatures = {}
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)      # macros go; a struct's members have no parentheses: no match below
    for ret, name, args in re.findall(r"([^;{}()]*?)\b(mm_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise NativeError(f"{name}: cannot bind the return type {ret!r}")
        argtypes = []
        for arg in [a.strip() for a in args.split(",") if args.strip() not in ("", "void")]:
            m = re.fullmatch(r"(?:const\s+)?(\w+)(?:\s+\w+)?", arg)
            if "*" not in arg and not (m and m.group(1) in _SCALARS):
                raise NativeError(f"{name}: cannot bind the argument {arg!r}")
            argtypes.append(ctypes.c_void_p if "*" in arg else _SCALARS[m.group(1)])
        signatures[name] = (_RETURNS[ret], argtypes)
    return signatures, defines


try:
    with open(HEADER_PATH) as _f:
        SIGNATURES, _DEFINES = _read_header(_f.read())
except OSError as e:
    raise NativeError(f"the C ABI is read from {os.path.normpath(HEADER_PATH)}, which cannot be opened: {e}") from e
# the header's constants under the names this package uses: MM_<NAME>, most of them without the prefix
for _name in ("MM_F32 MM_F16 MM_BF16 MASK_NONE MASK_LEN_I32 MASK_U8 MASK_I64 MASK_F32 TKL_SAT_EMBEDDING TKL_SAT_LOG SIM_ROUND SUM_ROUND "
              "STORE_KEEP_ZERO_ROWS ABI_VERSION MM_OK MM_EINVAL MM_EUNSUPPORTED MM_EWORKSPACE MM_ELAUNCH "
              "RANK_MAX_LEN RANK_MAX_CUTOFFS RANK_NOT_JUDGED DISTINCT_MAX_HITS "
              "PAIR_RANKNET PAIR_MARGIN PAIR_MARGIN_MSE PAIR_MSE_POINTWISE PAIR_KLDIV_POINTWISE PAIR_RANKNET_TEACHER PAIR_MSE_RANKNET "
              "LIST_LISTNET LIST_KLDIV LIST_SMOOTH_MRR LIST_LAMBDA_NDCG2 LIST_LAMBDA_NDCG2_TEACHER LOSS_MAX_LIST "
              "INBATCH_PAIR INBATCH_LIST").split():
    globals()[_name] = _DEFINES[_name if _name in _DEFINES else "MM_" + _name]

_lib = None


def lib():
    """Loads the shared library once; raises if it was not built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: build it with `python -m matchmaker_amd.build` "
                "(matchmaker_amd has no CPU / eager fallback for the scoring path)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        if L.mm_abi_version() != ABI_VERSION:
            raise NativeError(f"{LIB_PATH} has ABI version {L.mm_abi_version()}, this binding needs {ABI_VERSION}: "
                              "rebuild with `python -m matchmaker_amd.build --force`")
        _lib = L
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = lib().mm_last_error().decode("utf-8", "replace")
        raise NativeError(f"{what} failed ({code}): {msg}", code)
