"""MaxP dense retrieval: the step between a passage search and the ranked documents (`maxP->bert_dot`,
matchmaker/models/max_p_adapter.py:109-151 encodes one vector per passage, dense_retrieval.py:237-265 indexes them all under
their document's id, dense_retrieval.py:414-429 walks every query's hits on the host and keeps the first hit per id).

    distinct_hits(scores, ids, top_n) -> (scores, ids, pos, n_distinct, n_valid)      native mm_distinct_hits_fwd, DESIGN §3.23

The torch <-> ABI wrapper lives here, not in ops.py (ops.distinct_hits forwards to it); the module has its own `torch`,
`_workspace` and `clear_workspaces` names and allocates its outputs with `torch.empty`, so tests/poison.py can be pointed at it.
retrieval.MaxPIndexer is the indexer built on it.
"""
import torch

from . import _lib
from ._lib import NativeError
from .ops import _call, _dev_check, _workspace, clear_workspaces  # noqa: F401  (re-exported: tests/poison.py patches them here)

DISTINCT_MAX_HITS = _lib.DISTINCT_MAX_HITS      # hits per query of mm_distinct_hits_fwd (128 KB of 16-byte keys in LDS)


def _check(scores, ids, top_n):
    if scores.dim() != 2 or scores.dtype != torch.float32 or ids.dtype != torch.int64 or tuple(ids.shape) != tuple(scores.shape):
        raise NativeError(f"distinct_hits: scores must be float32 [nq, K] and ids int64 [nq, K], got {scores.dtype} "
                          f"{tuple(scores.shape)} and {ids.dtype} {tuple(ids.shape)}")
    nq, K = scores.shape
    top_n = int(top_n)
    if not 1 <= K <= DISTINCT_MAX_HITS:
        raise NativeError(f"distinct_hits: {K} hits per query outside 1 .. {DISTINCT_MAX_HITS}", _lib.MM_EUNSUPPORTED)
    if not 1 <= top_n <= K:
        raise NativeError(f"distinct_hits: top_n={top_n} outside 1 .. K={K}", _lib.MM_EUNSUPPORTED)
    if nq >= 1 << 31:
        raise NativeError(f"distinct_hits: nq={nq} >= 2^31", _lib.MM_EUNSUPPORTED)
    return nq, K, top_n


def distinct_hits(scores: torch.Tensor, ids: torch.Tensor, top_n: int):
    """Passage hits -> distinct documents (the `maxP->bert_dot` branch of the search loop, matchmaker/dense_retrieval.py:414-429;
    native mm_distinct_hits_fwd).

    scores [nq, K] float32 and ids [nq, K] int64 in the order the search returned them (descending; the list is not
    re-sorted).  Per query the first occurrence of every id >= 0 in list order is kept; ids < 0 are no hits.  Returns
    (scores [nq, top_n] float32, ids [nq, top_n] int64, pos [nq, top_n] int32 = the kept hit's position in the list, with
    -inf / -1 / -1 behind the kept hits, n_distinct [nq] int32 = distinct valid ids of the whole list, n_valid [nq] int32).
    1 <= top_n <= K <= DISTINCT_MAX_HITS.  One enqueue on the current stream, no workspace, no read-back: graph-capturable."""
    dev = _dev_check(scores, ids)
    nq, K, top_n = _check(scores, ids, top_n)
    scores, ids = scores.contiguous(), ids.contiguous()
    out_s = torch.empty((nq, top_n), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, top_n), dtype=torch.int64, device=dev)
    out_p = torch.empty((nq, top_n), dtype=torch.int32, device=dev)
    n_distinct = torch.empty(nq, dtype=torch.int32, device=dev)
    n_valid = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq == 0:
        return out_s, out_i, out_p, n_distinct, n_valid
    _call(dev, _lib.lib().mm_distinct_hits_fwd, (scores.data_ptr(), ids.data_ptr(), nq, K, top_n, out_s.data_ptr(),
                                                 out_i.data_ptr(), out_p.data_ptr(), n_distinct.data_ptr(),
                                                 n_valid.data_ptr()), stream_only=True)
    return out_s, out_i, out_p, n_distinct, n_valid
