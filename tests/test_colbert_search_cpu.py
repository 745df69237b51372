"""CPU tests of ColBERT end-to-end retrieval (TokenStore.search): the numpy restatement against hand-made cases, the sorted
view of the store, the C ABI declarations, the fake-tensor rule, and search() driven through stand-ins for its four native
calls (token search, candidates, MaxSim, selection)."""
import os

import numpy as np
import pytest
import torch

from tests import colbert_search_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the restatement itself
def test_candidates_ref_on_hand_made_cases():
    #            doc 0    doc 1 (empty)  doc 2     doc 3 (after a gap)
    begin, end = [0, 4, 4, 9], [4, 4, 7, 12]
    hits = [[0, 3, 3, -1],          # first and last row of doc 0, a repeat, no hit
            [4, 6, 11, 1],          # doc 2 shares its begin with the empty doc 1; last row of the last doc
            [7, 8, 12, 17],         # the gap 7..8 and rows past the store
            [-1, -7, -1, -1]]
    assert R.candidates_ref(hits, begin, end) == [[0], [0, 2, 3], [], []]
    assert R.candidates_ref_fast(hits, begin, end) == R.candidates_ref(hits, begin, end)
    doc, b, e, count = R.padded_candidates(R.candidates_ref(hits, begin, end), begin, end, 4)
    assert doc.tolist() == [[0, -1, -1, -1], [0, 2, 3, -1], [-1] * 4, [-1] * 4]
    assert b.tolist()[1] == [0, 4, 9, 0] and e.tolist()[1] == [4, 7, 12, 0] and count.tolist() == [1, 3, 0, 0]
    # documents whose seq_ids order is not their row order: still ascending by document index
    assert R.candidates_ref([[0, 5]], [4, 0], [8, 4]) == [[0, 1]]
    assert R.sorted_view([4, 0, 2], [8, 4, 2])[2].tolist() == [1, 0]            # the empty document is left out


def test_search_ref_on_a_hand_made_store():
    """3 documents of unit vectors, E = 4: the ranking can be read off by hand."""
    e = np.eye(4, dtype=np.float32)
    tokens = np.stack([e[0], e[1],          # doc 0
                       e[0] * 2,            # doc 1
                       e[2], e[1] * 3])     # doc 2
    begin, end = [0, 2, 3], [2, 3, 5]
    q = np.stack([np.stack([e[0], e[1], np.zeros(4, np.float32)])])      # one query: tokens e0, e1 and a dead one
    hits = R.token_hits_ref(q, tokens, 1)
    assert hits.tolist() == [[2, 4, -1]]                                  # best row per live token, -1 for the dead token
    s, d, cands = R.search_ref(q, tokens, begin, end, 1, 4, sim_round=True)
    assert cands == [[1, 2]]
    # doc 1: max(e0) = 2, max(e1) = 0, dead 0 -> 2 ; doc 2: 0 + 3 + 0 = 3
    assert d.tolist() == [[2, 1, -1, -1]] and s.tolist() == [[3.0, 2.0, -np.inf, -np.inf]]
    # k' = 2: ties at score 0 go to the lower row, so token e0 adds row 0 (doc 0: 1 + 1 = 2, ties doc 1 at 2: lower index first)
    s, d, cands = R.search_ref(q, tokens, begin, end, 2, 2, sim_round=False)
    assert R.token_hits_ref(q, tokens, 2).tolist() == [[2, 0, 4, 1, -1, -1]]
    assert cands == [[0, 1, 2]] and d.tolist() == [[2, 0]] and s.tolist() == [[3.0, 2.0]]


def test_exact_store_is_exact_and_its_order_is_decided_by_the_tie_rules():
    """The end-to-end GPU test compares bits on this store, so no arithmetic noise may exist on it: every inner product is an
    integer multiple of 1/64 below 2^9 (exact in fp32 in any summation order); fp16 rounding of such a value is one
    deterministic RNE step and leaves a multiple of 1/64, so the fp32 sums of the maxima are exact as well.  What is left to
    decide is ties, and those are decided by the stated rules: the restatement's k'-th boundary equals the order by
    (-score, row) computed in exact integer arithmetic, and its final order equals the order by (-score, document)."""
    c = R.exact_case()
    q, tokens, begin, end = c["q"], c["tokens"], c["begin"], c["end"]
    T = tokens.shape[0]
    assert len(begin) == 200 and (end - begin).min() >= 1 and (end - begin).max() <= 40 and T <= 4096
    assert np.array_equal(tokens * 8, np.round(tokens * 8)) and np.abs(tokens).max() <= 2
    assert np.array_equal(q * 8, np.round(q * 8)) and np.abs(q).max() <= 2
    assert [int((np.abs(q[i]).sum(-1) == 0).sum()) for i in range(q.shape[0])] == [2] * 5
    ti, qi = np.round(tokens * 8).astype(np.int64), np.round(q * 8).astype(np.int64)
    hits = R.token_hits_ref(q, tokens, c["k"])
    boundary_ties = 0
    for i in range(q.shape[0]):
        for t in range(q.shape[1]):
            got = hits[i, t * c["k"]: (t + 1) * c["k"]]
            if not qi[i, t].any():
                assert (got == -1).all()
                continue
            s = ti @ qi[i, t]                                   # 64 x the inner product, exact
            assert np.abs(s).max() < 512 * 64
            order = np.lexsort((np.arange(T), -s))
            assert np.array_equal(got, order[: c["k"]])
            boundary_ties += int(s[order[c["k"] - 1]] == s[order[c["k"]]])
    scores, idx, cands = R.search_ref(q, tokens, begin, end, c["k"], c["top_n"], sim_round=True, hit_rows=hits)
    final_ties = 0
    for i in range(q.shape[0]):
        # exact integer MaxSim with the fp16 rounding of every maximum
        exact = []
        for d in cands[i]:
            m = (ti[begin[d]: end[d]] @ qi[i].T).max(0) / 64.0
            exact.append((-float(m.astype(np.float16).astype(np.float64).sum()), d))
        exact.sort()
        n = min(c["top_n"], len(exact))
        assert [d for _, d in exact[:n]] == idx[i, :n].tolist()
        assert [-s for s, _ in exact[:n]] == scores[i, :n].tolist()
        final_ties += sum(exact[j][0] == exact[j + 1][0] for j in range(len(exact) - 1))
    print(f"exact store: T={T}, {boundary_ties} ties at a k'-th boundary, {final_ties} tied neighbours in the final orders")


# ------------------------------------------------------------------------------------------ the store's sorted view
def _store(begin, end, T=None, ids=None, **kw):
    from matchmaker_amd.token_store import TokenStore
    T = int(max(end)) if T is None else T
    return TokenStore(torch.zeros(T, 8, dtype=torch.float16), ids if ids is not None else [f"d{i}" for i in range(len(begin))],
                      np.array(begin), np.array(end), **kw)


def test_sorted_view_gaps_zero_length_and_permuted_documents():
    #           d0 rows 10..14, d1 empty at 3, d2 rows 0..3, d3 rows 3..7 (shares its begin with d1), gap 7..10, d4 empty inside d0
    st = _store([10, 3, 0, 3, 12], [14, 3, 3, 7, 12], T=20)
    assert st._begin_sorted.tolist() == [0, 3, 10] and st._end_sorted.tolist() == [3, 7, 14]
    assert st._doc_of_sorted.tolist() == [2, 3, 0] and st._doc_of_sorted.dtype == torch.int32
    assert st._begin_sorted.dtype == torch.int64 and st._end_sorted.dtype == torch.int64
    b, e, o = R.sorted_view([10, 3, 0, 3, 12], [14, 3, 3, 7, 12])
    assert (b.tolist(), e.tolist(), o.tolist()) == ([0, 3, 10], [3, 7, 14], [2, 3, 0])
    empty = _store([2, 2], [2, 2], T=4)                                    # nothing but zero-length documents
    assert empty._begin_sorted.numel() == 0


def test_overlapping_documents_are_refused_by_name():
    from matchmaker_amd import NativeError
    with pytest.raises(NativeError, match=r"'left'.*'right'.*overlap"):
        _store([0, 6, 4], [4, 9, 7], ids=["a", "right", "left"])       # rows 6 of "left" (4..7) and "right" (6..9)
    with pytest.raises(NativeError, match="overlap"):
        _store([0, 0], [4, 4])                                             # the same range twice
    _store([0, 4], [4, 8])                                                 # touching ranges do not overlap


# ------------------------------------------------------------------------------------------ C ABI and the torch op
def test_header_and_binding_declare_the_candidate_entry_points():
    from matchmaker_amd import _lib, build
    from tests import abi
    L = abi.assert_bound(("mm_colbert_candidates_workspace_bytes", "mm_colbert_candidates"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    assert _lib.ABI_VERSION == 4
    assert "dense_retrieval.py:391-412" in hdr and "colbert.py:100-112" in hdr
    assert "colbert_candidates.hip" in build.SOURCES
    # host arithmetic and refusals: callable without a GPU, nothing is launched
    assert L.mm_colbert_candidates_workspace_bytes(3, 1000) >= 3 * 1000 * 4
    assert L.mm_colbert_candidates_workspace_bytes(3, 16385) == 0
    p = 4096                                                               # any non-null value: refused before it is used
    assert L.mm_colbert_candidates(None, p, p, p, 5, 10, 1, 8, 5, p, p, p, p, p, 1 << 20, None) == _lib.MM_EINVAL
    assert L.mm_colbert_candidates(p, p, p, p, 5, 10, -1, 8, 5, p, p, p, p, p, 1 << 20, None) == _lib.MM_EINVAL
    assert L.mm_colbert_candidates(p, p, p, p, 5, 10, 1, 16385, 5, p, p, p, p, p, 1 << 20, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_colbert_candidates(p, p, p, p, 5, 10, 1, 8, 4, p, p, p, p, p, 1 << 20, None) == _lib.MM_EUNSUPPORTED
    assert L.mm_colbert_candidates(p, p, p, p, 1 << 31, 10, 1, 8, 8, p, p, p, p, p, 1 << 20, None) == _lib.MM_EUNSUPPORTED
    assert b"C_cap" in L.mm_last_error() or b"n_docs" in L.mm_last_error()


def test_ops_colbert_candidates_refuses_cpu_tensors_and_bad_arguments():
    from matchmaker_amd import ops, NativeError
    hits = torch.zeros(2, 4, dtype=torch.int64)
    b, e, o = torch.zeros(3, dtype=torch.int64), torch.ones(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(NativeError, match="CPU"):
        ops.colbert_candidates(hits, b, e, o, 3)


@pytest.mark.parametrize("nq, H, n_docs, c_cap, C", [(5, 128, 1000, None, 128), (2, 4096, 50, None, 50), (3, 16, 9, 40, 40), (0, 7, 7, None, 7)])
def test_fake_tensor_rule_of_the_torch_op(nq, H, n_docs, c_cap, C):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        hits = torch.empty(nq, H, dtype=torch.int64, device="cuda")
        b = torch.empty(n_docs, dtype=torch.int64, device="cuda")
        o = torch.empty(n_docs, dtype=torch.int32, device="cuda")
        doc, cb, ce, count = torch.ops.mm_native.colbert_candidates(hits, b, b, o, 12345, c_cap)
        assert doc.shape == cb.shape == ce.shape == (nq, C) and count.shape == (nq,)
        assert (doc.dtype, cb.dtype, ce.dtype, count.dtype) == (torch.int32, torch.int64, torch.int64, torch.int32)
        assert doc.device.type == "cuda" and not doc.requires_grad


# ------------------------------------------------------------------------------------------ search() through stand-ins
class _StandIns:
    """torch-on-CPU versions of the four native calls, with the operators' contracts; they record how they were called."""

    def __init__(self):
        self.topk_rows, self.cand_shapes, self.maxsim_C = [], [], []

    def topk(self, queries, matrix, k):
        self.topk_rows.append(queries.shape[0])
        assert queries.dtype == matrix.dtype and (queries != 0).any(dim=1).all(), "only live tokens are searched"
        s = queries.double() @ matrix.double().T
        order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
        scores = torch.full((queries.shape[0], k), float("-inf"))
        idx = torch.full((queries.shape[0], k), -1, dtype=torch.int64)
        idx[:, : order.shape[1]] = order
        scores[:, : order.shape[1]] = torch.gather(s, 1, order).float()
        return scores, idx

    def candidates(self, hit_rows, bs, es, dof, T, c_cap):
        self.cand_shapes.append((tuple(hit_rows.shape), c_cap))
        begin, end = {}, {}
        for b, e, d in zip(bs.tolist(), es.tolist(), dof.tolist()):
            begin[d], end[d] = b, e
        n = max(begin) + 1
        bl, el = [begin.get(d, 0) for d in range(n)], [end.get(d, 0) for d in range(n)]
        out = R.padded_candidates(R.candidates_ref(hit_rows.numpy(), bl, el), bl, el, c_cap)
        return tuple(torch.from_numpy(x) for x in out)

    def maxsim(self, q, tokens, b, e, q_mask, pairs_per_query, check_ranges, sim_round):
        assert q_mask is None and check_ranges is False and q.dtype == tokens.dtype
        self.maxsim_C.append(pairs_per_query)
        out = torch.empty(b.numel(), dtype=torch.float32)
        for p in range(b.numel()):
            doc = tokens[int(b[p]): int(e[p])].float().numpy()
            out[p] = float(R.maxsim_ref(q[p // pairs_per_query].float().numpy(), doc, sim_round)) if doc.shape[0] else -1000.0 * q.shape[1]
        return out

    def merge(self, scores, ids, k):
        s = torch.where(ids >= 0, scores, torch.full_like(scores, float("-inf")))
        order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
        out_s = torch.full((s.shape[0], k), float("-inf"))
        out_i = torch.full((s.shape[0], k), -1, dtype=torch.int64)
        out_s[:, : order.shape[1]] = torch.gather(s, 1, order)
        out_i[:, : order.shape[1]] = torch.gather(ids, 1, order)
        out_i[out_s == float("-inf")] = -1
        return out_s, out_i


def _exact_store_on_cpu(fn, permute=False):
    from matchmaker_amd.token_store import TokenStore
    c = R.exact_case()
    n = len(c["begin"])
    ids = [f"doc{i}" for i in range(n)]
    st = TokenStore(torch.from_numpy(c["tokens"]).half(), ids, c["begin"], c["end"], topk_fn=fn.topk, candidates_fn=fn.candidates,
                    maxsim_fn=fn.maxsim, merge_fn=fn.merge)
    return c, st, ids


@pytest.mark.parametrize("use_fp16", [True, False])
def test_search_through_stand_ins_matches_the_restatement(use_fp16):
    fn = _StandIns()
    c, st, ids = _exact_store_on_cpu(fn)
    q = torch.from_numpy(c["q"])
    nq, Q, _ = q.shape
    ref_s, ref_d, cands = R.search_ref(c["q"], c["tokens"], c["begin"], c["end"], c["k"], c["top_n"], sim_round=use_fp16)
    s, d = st.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert s.dtype == torch.float32 and d.dtype == torch.int64 and s.shape == d.shape == (nq, c["top_n"])
    assert np.array_equal(d.numpy(), ref_d) and np.array_equal(s.numpy(), ref_s)
    # dead tokens are not searched: one call over the 6 live tokens of each of the 5 queries; their hit slots are -1
    assert fn.topk_rows == [nq * (Q - 2)]
    hits = st.token_hits(q, c["k"])
    assert np.array_equal(hits.numpy(), R.token_hits_ref(c["q"], c["tokens"], c["k"]))
    # candidate slots: min(H, documents) asked for, trimmed to the largest count before the MaxSim
    assert fn.cand_shapes[0] == ((nq, Q * c["k"]), min(Q * c["k"], 200))
    assert fn.maxsim_C == [max(len(x) for x in cands)]
    # trim=False keeps every slot and gives the same result
    s2, d2 = st.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16, trim=False)
    assert fn.maxsim_C[-1] == min(Q * c["k"], 200) and torch.equal(s2, s) and torch.equal(d2, d)
    # query_chunk bounds the tokens per token-search call
    fn.topk_rows.clear()
    s3, d3 = st.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16, query_chunk=7)
    assert fn.topk_rows == [7, 7, 7, 7, 2] and torch.equal(s3, s) and torch.equal(d3, d)
    # search(): (seq_id, score) lists, best first
    res = st.search(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert res == [[(ids[j], float(x)) for x, j in zip(ref_s[i], ref_d[i]) if j >= 0] for i in range(nq)]


def test_search_padding_dead_queries_and_the_hit_limit():
    from matchmaker_amd import NativeError
    fn = _StandIns()
    c, st, ids = _exact_store_on_cpu(fn)
    q = torch.from_numpy(c["q"]).clone()
    q[3] = 0                                                    # a query without a live token
    s, d = st.search_device(q, 150, 2, use_fp16=True)           # at most 6 x 2 candidates per query: a long (-inf, -1) tail
    ref_s, ref_d, cands = R.search_ref(q.numpy(), c["tokens"], c["begin"], c["end"], 2, 150, sim_round=True)
    assert np.array_equal(d.numpy(), ref_d) and np.array_equal(s.numpy(), ref_s)
    assert cands[3] == [] and (d[3] == -1).all() and torch.isinf(s[3]).all()
    assert all((d[i, len(cands[i]):] == -1).all() and (d[i, : len(cands[i])] >= 0).all() for i in range(5))
    assert st.search(q, 150, 2)[3] == []
    s0, d0 = st.search_device(torch.zeros_like(q), 4, 2)        # no live token at all: no token search, all padding
    assert (d0 == -1).all() and torch.isinf(s0).all()
    with pytest.raises(NativeError, match="16384"):
        st.search_device(q, 10, 16384 // q.shape[1] + 1)
    e0 = st.search_device(q[:0], 10, 4)
    assert e0[0].shape == (0, 10) and e0[1].shape == (0, 10)


def test_search_maps_permuted_seq_ids():
    """Documents whose seq_ids order is a permutation of their row order: doc_idx are positions in seq_ids and ties go to the
    lower position."""
    from matchmaker_amd.token_store import TokenStore
    fn = _StandIns()
    c = R.exact_case()
    n = len(c["begin"])
    perm = np.random.default_rng(9).permutation(n)
    begin, end = c["begin"][perm], c["end"][perm]
    ids = [f"p{i}" for i in range(n)]
    st = TokenStore(torch.from_numpy(c["tokens"]).half(), ids, begin, end, topk_fn=fn.topk, candidates_fn=fn.candidates,
                    maxsim_fn=fn.maxsim, merge_fn=fn.merge)
    ref_s, ref_d, _ = R.search_ref(c["q"], c["tokens"], begin, end, c["k"], c["top_n"], sim_round=True)
    s, d = st.search_device(torch.from_numpy(c["q"]), c["top_n"], c["k"])
    assert np.array_equal(d.numpy(), ref_d) and np.array_equal(s.numpy(), ref_s)
