"""References for the MaxP retrieval tests (a helper like tests/poison.py, not a test module).

distinct_hits: matchmaker/dense_retrieval.py:414-429 restated per query in plain Python — walk the hit list, keep a `set` of
ids, take the first hit of every id, stop at top_n — extended with what mm_distinct_hits_fwd adds: ids < 0 are no hits, the
fill values behind the kept hits, the kept hit's position and the two counts (which need the walk to go on to the list's end).

brute_force: the document ranking from nothing but the vectors, in float64: every passage's score, a stable descending
argsort (lower row first on equal scores), then the same loop over ALL passages."""
import numpy as np


def distinct_hits(scores, ids, top_n):
    """scores [nq, K] float32, ids [nq, K] int64 -> (scores [nq, top_n] float32, ids int64, pos int32, n_distinct [nq] int32,
    n_valid [nq] int32) as ops.distinct_hits returns them.  Scores are copied, never compared."""
    scores, ids = np.asarray(scores), np.asarray(ids)
    nq, K = ids.shape
    out_s = np.full((nq, top_n), -np.inf, dtype=np.float32)
    out_i = np.full((nq, top_n), -1, dtype=np.int64)
    out_p = np.full((nq, top_n), -1, dtype=np.int32)
    n_distinct = np.zeros(nq, dtype=np.int32)
    n_valid = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        unique_ids = set()
        kept = 0
        for t, s_idx in enumerate(ids[q].tolist()):
            if s_idx < 0:
                continue
            n_valid[q] += 1
            if s_idx in unique_ids:
                continue
            unique_ids.add(s_idx)
            if kept < top_n:
                out_s[q, kept], out_i[q, kept], out_p[q, kept] = scores[q, t], s_idx, t
                kept += 1
        n_distinct[q] = len(unique_ids)
    return out_s, out_i, out_p, n_distinct, n_valid


def topk_hits(queries, vectors, ids, k):
    """The exact passage search in float64: (scores [nq, k] float32, ids [nq, k] int64, rows [nq, k] int64), descending, lower
    row first on equal scores, -inf / -1 / -1 where the index holds fewer than k vectors."""
    s = np.asarray(queries, dtype=np.float64) @ np.asarray(vectors, dtype=np.float64).T
    nq, n = s.shape
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    m = min(k, n)
    out_s[:, :m] = np.take_along_axis(s, order, axis=1).astype(np.float32)
    out_i[:, :m] = np.asarray(ids, dtype=np.int64)[order]
    out_r[:, :m] = order
    return out_s, out_i, out_r


def brute_force(queries, vectors, ids, top_n):
    """The exact top_n documents of every query: distinct_hits over the whole ranked collection."""
    s, i, _ = topk_hits(queries, vectors, ids, np.asarray(vectors).shape[0])
    return distinct_hits(s, i, top_n)
