"""numpy restatement of ColBERT end-to-end retrieval (TokenStore.search), in plain loops.

For query i with token vectors q[i] [Q, E]:
  1. a query token is live if its vector has a non-zero element; dead tokens search nothing and add 0 to every MaxSim sum;
  2. every live token takes the exact top-k' rows of the token matrix by inner product (fp32 of the 16-bit values), equal
     scores to the lower row;
  3. the candidates are the documents that own at least one hit row (begin[d] <= row < end[d]); rows no document owns, hits
     of -1 and rows outside the matrix are dropped;
  4. every candidate is scored by forward_aggregation (colbert.py:100-112): per query token the maximum inner product over
     the document's rows (rounded to fp16 when sim_round, as under the searcher head's autocast), summed in fp32;
  5. the top_n candidates by score, equal scores to the lower document index; (-inf, -1) fills the rest.
"""
import numpy as np


def candidates_ref(hit_rows, begin, end):
    """hit_rows [nq, H] ints; begin / end [n_docs] in document (seq_ids) order.  Returns, per query, the ascending list of the
    documents that own at least one hit row."""
    out = []
    for hits in np.asarray(hit_rows):
        owners = set()
        for row in hits:
            row = int(row)
            if row < 0:
                continue
            for d in range(len(begin)):
                if begin[d] <= row < end[d]:
                    owners.add(d)
        out.append(sorted(owners))
    return out


def candidates_ref_fast(hit_rows, begin, end):
    """candidates_ref for large cases (300 queries x 16,384 hits x 5,000 documents): the same definition through a table
    row -> owning document, filled document by document (the ranges of non-empty documents must be disjoint)."""
    T = int(max(end)) if len(end) else 0
    owner = np.full(T, -1, dtype=np.int64)
    for d in range(len(begin)):
        owner[begin[d]: end[d]] = d
    out = []
    for hits in np.asarray(hit_rows):
        rows = hits[(hits >= 0) & (hits < T)]
        docs = np.unique(owner[rows])
        out.append(docs[docs >= 0].tolist())
    return out


def padded_candidates(cands, begin, end, c_cap):
    """The four arrays mm_colbert_candidates writes for the candidate lists `cands`."""
    nq = len(cands)
    doc = np.full((nq, c_cap), -1, dtype=np.int32)
    b = np.zeros((nq, c_cap), dtype=np.int64)
    e = np.zeros((nq, c_cap), dtype=np.int64)
    count = np.zeros(nq, dtype=np.int32)
    for i, c in enumerate(cands):
        count[i] = len(c)
        for s, d in enumerate(c):
            doc[i, s], b[i, s], e[i, s] = d, begin[d], end[d]
    return doc, b, e, count


def sorted_view(begin, end):
    """(begin_sorted, end_sorted, doc_of_sorted): the documents that hold rows, sorted by (begin, end)."""
    docs = [d for d in range(len(begin)) if end[d] > begin[d]]
    docs.sort(key=lambda d: (begin[d], end[d]))
    return (np.array([begin[d] for d in docs], dtype=np.int64), np.array([end[d] for d in docs], dtype=np.int64),
            np.array(docs, dtype=np.int32))


def token_hits_ref(q, tokens, k):
    """[nq, Q * k] int64: steps 1-2.  q [nq, Q, E], tokens [T, E]: float arrays holding the 16-bit values."""
    nq, Q, _ = q.shape
    T = tokens.shape[0]
    t64 = tokens.astype(np.float64)
    hits = np.full((nq, Q, k), -1, dtype=np.int64)
    for i in range(nq):
        for t in range(Q):
            if not np.any(q[i, t] != 0):
                continue
            s = (t64 @ q[i, t].astype(np.float64)).astype(np.float32)
            order = np.lexsort((np.arange(T), -s))[:k]         # score descending, then row ascending
            hits[i, t, : len(order)] = order
    return hits.reshape(nq, Q * k)


def maxsim_ref(qi, doc, sim_round):
    """forward_aggregation of one query [Q, E] against one document [n, E] (float32 result)."""
    total = np.float32(0)
    for t in range(qi.shape[0]):
        sims = (doc.astype(np.float64) @ qi[t].astype(np.float64)).astype(np.float32)
        if sim_round:
            sims = sims.astype(np.float16).astype(np.float32)
        total = np.float32(total + sims.max())
    return total


def search_ref(q, tokens, begin, end, k, top_n, sim_round, hit_rows=None):
    """(scores [nq, top_n] float32, doc_idx [nq, top_n] int64, candidates): steps 1-5.  hit_rows: token hits to start from
    instead of steps 1-2."""
    nq = q.shape[0]
    if hit_rows is None:
        hit_rows = token_hits_ref(q, tokens, k)
    cands = candidates_ref_fast(hit_rows, begin, end)
    scores = np.full((nq, top_n), -np.inf, dtype=np.float32)
    idx = np.full((nq, top_n), -1, dtype=np.int64)
    for i in range(nq):
        scored = [(maxsim_ref(q[i], tokens[begin[d]: end[d]], sim_round), d) for d in cands[i]]
        scored.sort(key=lambda sd: (-sd[0], sd[1]))
        for s, (sc, d) in enumerate(scored[:top_n]):
            scores[i, s], idx[i, s] = sc, d
    return scores, idx, cands


def exact_case(seed=5):
    """The store with exactly representable arithmetic of the end-to-end tests: 200 documents of 1-40 tokens, E 128, values
    multiples of 1/8 in [-2, 2] (every inner product is a multiple of 1/64 below 512: exact in fp32 whatever the summation
    order); 5 queries of 8 tokens, two of them zero rows; k' 16, top_n 10.  The seed is one whose store has at most 4,096
    token rows, so that a token search with k' >= T fits ops.dot_topk's k <= 4096."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 41, 200)
    end = np.cumsum(lens).astype(np.int64)
    begin = (end - lens).astype(np.int64)
    tokens = (rng.integers(-16, 17, (int(end[-1]), 128)) / 8.0).astype(np.float32)
    tokens[np.abs(tokens).sum(-1) == 0, 0] = 0.125            # a stored row is never all zero (dense_retrieval.py:244)
    q = (rng.integers(-16, 17, (5, 8, 128)) / 8.0).astype(np.float32)
    for i in range(5):
        q[i, rng.choice(8, 2, replace=False)] = 0
    return {"q": q, "tokens": tokens, "begin": begin, "end": end, "k": 16, "top_n": 10}
