"""ctypes binding of libmm_native.so (C ABI declared in include/mm_native.h).

There is NO fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# MM_NATIVE_LIB: another build of the same library for ONE process (A/B variants, tools/build_variant.sh)
LIB_PATH = os.environ.get("MM_NATIVE_LIB") or os.path.join(HERE, "csrc", "libmm_native.so")

MM_F32, MM_F16, MM_BF16 = 0, 1, 2
MASK_NONE, MASK_LEN_I32, MASK_U8, MASK_I64, MASK_F32 = 0, 1, 2, 3, 4
TKL_SAT_EMBEDDING, TKL_SAT_LOG = 0, 1
SIM_ROUND, SUM_ROUND = 1, 2          # MM_SIM_ROUND / MM_SUM_ROUND
STORE_KEEP_ZERO_ROWS = 1             # MM_STORE_KEEP_ZERO_ROWS
ABI_VERSION = 4
MM_OK, MM_EINVAL, MM_EUNSUPPORTED, MM_EWORKSPACE, MM_ELAUNCH = 0, -1, -2, -3, -4

_c = ctypes
_vp, _i64, _i, _sz = _c.c_void_p, _c.c_int64, _c.c_int, _c.c_size_t

# symbol -> (restype, argtypes): must list every function declared in include/mm_native.h
SIGNATURES = {
    "mm_abi_version": (_i, []),
    "mm_last_error": (_c.c_char_p, []),
    "mm_maxsim_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i, _i]),
    "mm_maxsim_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_maxsim_fwd_batched": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "mm_maxsim_inbatch_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i, _i]),
    "mm_maxsim_inbatch_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_maxsim_ragged_workspace_bytes": (_sz, [_i64, _i64, _i, _i]),
    "mm_maxsim_ragged_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_hbm_stream_probe": (_i, [_vp, _i64, _i, _vp]),
    "mm_maxsim_bwd_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_maxsim_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_maxsim_inbatch_bwd_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i, _i, _i]),
    "mm_maxsim_inbatch_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i, _i]),
    "mm_kernel_pool_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_ex_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _c.c_float, _vp, _vp, _i64, _i64,
                                   _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_ex_fwd2": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _c.c_float, _vp, _vp, _vp, _i64, _i64,
                                    _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_ex_bwd2": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _c.c_float, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_ex_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _c.c_float, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_tkl_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "mm_tkl_bwd_workspace_bytes2": (_sz, [_i64, _i, _i, _i]),
    "mm_tkl_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_multi_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i, _i, _i, _i]),
    "mm_kernel_pool_multi_fwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _c.c_float, _vp, _i64, _i64,
                                      _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_kernel_pool_bwd_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_kernel_pool_bwd_workspace_bytes2": (_sz, [_i64, _i, _i, _i, _i, _i]),
    "mm_kernel_pool_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_dot_topk_workspace_bytes": (_sz, [_i64, _i, _i]),
    "mm_dot_topk_fwd": (_i, [_vp, _vp, _i64, _i, _i, _i, _i, _c.c_float, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mm_topk_merge": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "mm_tkl_workspace_bytes": (_sz, [_i64, _i64, _i, _i, _i]),
    "mm_tkl_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_tkl_fwd_peaks": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_ivf_scan_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_ivf_scan_fwd": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mm_ah_encode": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _c.c_float, _i, _vp, _vp]),
    "mm_ah_scan_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_ah_scan_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mm_gather_dot": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _vp, _vp]),
    "mm_graph_search_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i, _i, _i]),
    "mm_graph_search_fwd": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mm_kmeans_assign": (_i, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp]),
    "mm_kmeans_segment_sum_workspace_bytes": (_sz, [_i64, _i, _i]),
    "mm_kmeans_segment_sum": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mm_pacrr_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i, _i]),
    "mm_pacrr_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_pacrr_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_co_pacrr_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i, _i, _i]),
    "mm_co_pacrr_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz,
                             _vp]),
    "mm_co_pacrr_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i,
                             _vp, _sz, _vp]),
    "mm_drmm_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_drmm_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_matchpyramid_workspace_bytes": (_sz, [_i64, _i, _i, _i, _vp]),
    "mm_matchpyramid_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mm_matchpyramid_fwd_save_workspace_bytes": (_sz, [_i64, _i, _i, _i, _vp]),
    "mm_matchpyramid_fwd_save": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mm_matchpyramid_bwd_workspace_bytes": (_sz, [_i64, _i, _i, _i, _vp]),
    "mm_matchpyramid_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _vp, _sz,
                                 _vp]),
    "mm_colbert_candidates_workspace_bytes": (_sz, [_i, _i]),
    "mm_colbert_candidates": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mm_fp8_quantize_rows": (_i, [_vp, _i64, _i, _i, _vp, _vp, _vp]),
    "mm_maxsim_ragged_fp8_workspace_bytes": (_sz, [_i64, _i64, _i, _i]),
    "mm_maxsim_ragged_fp8_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i64, _i64, _i, _i, _i, _i, _vp, _sz, _vp]),
    "mm_dot_topk_fp8_workspace_bytes": (_sz, [_i64, _i, _i]),
    "mm_dot_topk_fp8_fwd": (_i, [_vp, _vp, _vp, _i64, _i, _i, _i, _i, _c.c_float, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mm_ivf_scan_fp8_workspace_bytes": (_sz, [_i64, _i, _i, _i, _i]),
    "mm_ivf_scan_fp8_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "mm_store_append_workspace_bytes": (_sz, [_i, _i]),
    "mm_store_append": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mm_segment_rank_fwd": (_i, [_vp, _i, _vp, _i64, _i, _i, _vp, _vp]),
    "mm_rank_metrics_fwd": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _c.c_double, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i,
                                 _vp, _vp, _vp, _vp, _vp]),
    "mm_rank_metrics_depth_fwd": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _c.c_double, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _i,
                                       _vp, _vp, _vp, _vp, _vp]),
}
RANK_MAX_LEN, RANK_MAX_CUTOFFS, RANK_NOT_JUDGED = 8192, 8, -2 ** 31      # MM_RANK_MAX_LEN / _MAX_CUTOFFS / _NOT_JUDGED

_lib = None


class NativeError(RuntimeError):
    """.code: the C return code (MM_E*) when the error came from libmm_native.so or restates one of its checks, else None."""

    def __init__(self, msg="", code=None):
        super().__init__(msg)
        self.code = code


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
