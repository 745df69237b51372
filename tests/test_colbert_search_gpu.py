"""GPU tests of ColBERT end-to-end retrieval: the candidate kernel (mm_colbert_candidates) against the numpy restatement,
exact equality of all four outputs, and TokenStore.search end to end (tests/colbert_search_reference.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import colbert_search_reference as R
from tests import util

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the candidate kernel
def _layout(rng, n_docs, permute=True, gaps=True, empties=True):
    """A store layout in document (seq_ids) order: lengths 1..40, optional gaps between documents, zero-length documents that
    share their begin with the next document, seq_ids order a permutation of the row order.  Returns (begin, end, T)."""
    lens = rng.integers(1, 41, n_docs)
    if empties and n_docs >= 3:
        lens[rng.choice(n_docs, n_docs // 5, replace=False)] = 0
        lens[0] = max(lens[0], 1)
    gap = rng.integers(0, 4, n_docs) if gaps else np.zeros(n_docs, dtype=np.int64)
    begin = np.cumsum(lens + gap) - lens
    end = begin + lens
    T = int(end.max()) + int(rng.integers(0, 3))
    if permute:
        p = rng.permutation(n_docs)
        begin, end = begin[p], end[p]
    return begin.astype(np.int64), end.astype(np.int64), T


def _run_kernel(hits, begin, end, T, c_cap=None):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    bs, es, dof = R.sorted_view(begin, end)
    out = ops.colbert_candidates(torch.from_numpy(np.ascontiguousarray(hits)).to(dev), torch.from_numpy(bs).to(dev),
                                 torch.from_numpy(es).to(dev), torch.from_numpy(dof).to(dev), T, c_cap)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out], len(bs)


def _check_kernel(hits, begin, end, T, c_cap=None, ref=R.candidates_ref_fast):
    hits = np.asarray(hits, dtype=np.int64)
    got, n_sorted = _run_kernel(hits, begin, end, T, c_cap)
    cap = min(hits.shape[1], n_sorted) if c_cap is None else c_cap
    want = R.padded_candidates(ref(hits, begin, end), begin, end, cap)
    for name, g, w in zip(("cand_doc", "cand_begin", "cand_end", "count"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())
    return got


@pytest.mark.parametrize("n_docs", [1, 3, 5000])
@pytest.mark.parametrize("nq", [1, 300])
@pytest.mark.parametrize("H", [1, 63, 65, 1000, 16384])
def test_kernel_matches_the_restatement_over_hit_counts(H, nq, n_docs):
    """Sorts that are no power of two, one and many wavefronts, more queries than workgroups (grid stride); hits anywhere in
    [-3, T + 5): -1 and negative rows, gaps, rows past the store."""
    rng = np.random.default_rng(H * 1000 + nq + n_docs)
    begin, end, T = _layout(rng, n_docs)
    hits = rng.integers(-3, T + 5, (nq, H))
    hits[rng.random((nq, H)) < 0.1] = -1
    got = _check_kernel(hits, begin, end, T)
    if H >= 1000 and n_docs == 5000:
        assert got[3].min() > 256                               # a real load: hundreds of distinct documents per query


def test_kernel_small_cases_by_the_plain_loop_restatement():
    """The plain-loop candidates_ref (no table) on a case small enough for it."""
    rng = np.random.default_rng(4)
    begin, end, T = _layout(rng, 40)
    _check_kernel(rng.integers(-2, T + 3, (7, 90)), begin, end, T, ref=R.candidates_ref)


def test_kernel_all_hits_missing():
    begin, end, T = _layout(np.random.default_rng(1), 50)
    doc, b, e, count = _check_kernel(np.full((3, 200), -1), begin, end, T)
    assert (count == 0).all() and (doc == -1).all() and (b == 0).all() and (e == 0).all()


def test_kernel_all_hits_in_one_document():
    begin, end, T = _layout(np.random.default_rng(2), 50, empties=False)
    d = 17
    hits = np.random.default_rng(3).integers(begin[d], end[d], (2, 777))
    doc, _, _, count = _check_kernel(hits, begin, end, T)
    assert count.tolist() == [1, 1] and doc[:, 0].tolist() == [d, d]


def test_kernel_all_hits_distinct_with_exactly_h_slots():
    rng = np.random.default_rng(5)
    begin, end, T = _layout(rng, 5000, empties=False)
    H = 257
    docs = np.stack([rng.choice(5000, H, replace=False) for _ in range(3)])
    hits = begin[docs] + rng.integers(0, 1 << 30, docs.shape) % (end[docs] - begin[docs])
    doc, _, _, count = _check_kernel(hits, begin, end, T, c_cap=H)
    assert count.tolist() == [H] * 3 and (doc >= 0).all()


def test_kernel_boundary_rows_and_rows_outside_the_store():
    begin, end, _ = _layout(np.random.default_rng(6), 30, permute=False, gaps=False, empties=False)
    T = int(end[-1])                                            # the last document ends the store
    hits = np.array([[0, T - 1, T, T + 5, -7, -1, 2 ** 40, -2 ** 40]])
    doc, _, _, count = _check_kernel(hits, begin, end, T)
    assert count.tolist() == [2] and doc[0, :2].tolist() == [0, 29]


def test_kernel_gaps_between_documents():
    begin = np.array([2, 10, 20], dtype=np.int64)
    end = np.array([5, 12, 21], dtype=np.int64)
    hits = np.array([[0, 1, 5, 9, 12, 19, 21, 24], [4, 5, 6, 10, 20, 19, 1, 0]])
    doc, b, e, count = _check_kernel(hits, begin, end, 25)
    assert count.tolist() == [0, 3] and doc[1].tolist() == [0, 1, 2] and b[1].tolist() == [2, 10, 20] and e[1].tolist() == [5, 12, 21]


def test_kernel_zero_length_documents_never_own_a_row():
    """Handed to the kernel itself (the store leaves them out of its sorted view): zero-length ranges that share their begin
    with a real document, in front of it in (begin, end) order."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    bs = torch.tensor([0, 0, 0, 4, 4, 9, 9], dtype=torch.int64, device=dev)
    es = torch.tensor([0, 0, 4, 4, 9, 9, 9], dtype=torch.int64, device=dev)      # documents 2 and 4 hold the rows
    dof = torch.tensor([6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device=dev)
    hits = torch.tensor([[0, 3, 4, 8, 9, -1]], dtype=torch.int64, device=dev)
    doc, b, e, count = ops.colbert_candidates(hits, bs, es, dof, 9)
    assert count.tolist() == [2] and doc.tolist() == [[2, 4, -1, -1, -1, -1]]
    assert b.tolist() == [[4, 0, 0, 0, 0, 0]] and e.tolist() == [[9, 4, 0, 0, 0, 0]]


def test_kernel_permuted_seq_ids_give_ascending_document_indices():
    rng = np.random.default_rng(8)
    begin, end, T = _layout(rng, 500, permute=True, empties=False)
    doc, b, e, count = _check_kernel(rng.integers(0, T, (4, 300)), begin, end, T)
    for i in range(4):
        row = doc[i, : count[i]]
        assert (np.diff(row) > 0).all() and np.array_equal(b[i, : count[i]], begin[row]) and np.array_equal(e[i, : count[i]], end[row])


def test_kernel_refusals_launch_nothing():
    from matchmaker_amd import ops, _lib, NativeError
    dev = util.require_gpu()
    bs = torch.arange(0, 50, 5, dtype=torch.int64, device=dev)
    es = bs + 5
    dof = torch.arange(10, dtype=torch.int32, device=dev)
    with pytest.raises(NativeError) as ei:
        ops.colbert_candidates(torch.zeros(1, 16385, dtype=torch.int64, device=dev), bs, es, dof, 50)
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError) as ei:
        ops.colbert_candidates(torch.zeros(1, 8, dtype=torch.int64, device=dev), bs, es, dof, 50, c_cap=7)
    assert ei.value.code == _lib.MM_EUNSUPPORTED
    # the C entry point itself: outputs stay as they were
    L = _lib.lib()
    hits = torch.zeros(2, 8, dtype=torch.int64, device=dev)
    out = [torch.full((2, 8), 77, dtype=torch.int32, device=dev), torch.full((2, 8), 77, dtype=torch.int64, device=dev),
           torch.full((2, 8), 77, dtype=torch.int64, device=dev), torch.full((2,), 77, dtype=torch.int32, device=dev)]
    big = torch.zeros(2 * 16385, dtype=torch.int64, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    ptr = [t.data_ptr() for t in out]

    def call(h, H, c_cap, hits_ptr=None, cand_doc=ptr[0]):
        return L.mm_colbert_candidates(h.data_ptr() if hits_ptr is None else hits_ptr, bs.data_ptr(), es.data_ptr(), dof.data_ptr(),
                                       10, 50, 2, H, c_cap, cand_doc, ptr[1], ptr[2], ptr[3], ws.data_ptr(), ws.numel(), None)

    assert call(big, 16385, 8) == _lib.MM_EUNSUPPORTED
    assert call(hits, 8, 7) == _lib.MM_EUNSUPPORTED
    assert call(hits, 8, 8, cand_doc=None) == _lib.MM_EINVAL
    assert L.mm_colbert_candidates(None, bs.data_ptr(), es.data_ptr(), dof.data_ptr(), 10, 50, 2, 8, 8, *ptr, ws.data_ptr(),
                                   ws.numel(), None) == _lib.MM_EINVAL
    assert L.mm_colbert_candidates(hits.data_ptr(), bs.data_ptr(), es.data_ptr(), dof.data_ptr(), 10, 50, 2, 8, 8, *ptr, None, 0,
                                   None) == _lib.MM_EWORKSPACE
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out)
    assert call(hits, 8, 8) == _lib.MM_OK                        # and the same arguments inside the envelope run
    torch.cuda.synchronize()
    assert out[3].tolist() == [1, 1] and out[0][:, 0].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ end to end, exact arithmetic
@functools.lru_cache(maxsize=None)
def _exact():
    """The exact store, its restatement results (computed once, never modified) and its device stores."""
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    c = R.exact_case()
    ids = [f"doc{i}" for i in range(len(c["begin"]))]
    hits = R.token_hits_ref(c["q"], c["tokens"], c["k"])
    ref = {sr: R.search_ref(c["q"], c["tokens"], c["begin"], c["end"], c["k"], c["top_n"], sim_round=sr, hit_rows=hits)
           for sr in (True, False)}
    st16 = TokenStore(torch.from_numpy(c["tokens"]).half().to(dev), ids, c["begin"], c["end"])
    return c, ids, hits, ref, st16


@pytest.mark.parametrize("use_fp16", [True, False])
def test_search_is_bit_equal_to_the_restatement_on_the_exact_store(use_fp16):
    """nq 5, Q 8 (two zero rows per query), k' 16, top_n 10 on the fp16 store of 200 documents with exactly representable
    arithmetic: token hits, candidates, document order and scores equal the restatement bit for bit — no tolerance.  (The inner
    products reach beyond fp16's exact range of multiples of 1/64, so use_fp16 does round maxima; that rounding is one RNE step of
    an exactly known value, the same in numpy, and the sums stay exact: tests/test_colbert_search_cpu.py.)"""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c, ids, hits, ref, st = _exact()
    q = torch.from_numpy(c["q"]).half().to(dev)
    got_hits = st.token_hits(q, c["k"])
    assert np.array_equal(got_hits.cpu().numpy(), hits)
    cand = ops.colbert_candidates(got_hits, st._begin_sorted, st._end_sorted, st._doc_of_sorted, st.tokens.shape[0])
    want = R.padded_candidates(ref[use_fp16][2], c["begin"], c["end"], cand[0].shape[1])
    for g, w in zip(cand, want):
        assert np.array_equal(g.cpu().numpy(), w)
    s, d = st.search_device(q, c["top_n"], c["k"], use_fp16=use_fp16)
    assert s.dtype == torch.float32 and d.dtype == torch.int64
    assert np.array_equal(d.cpu().numpy(), ref[use_fp16][1])
    assert np.array_equal(s.cpu().numpy(), ref[use_fp16][0])


def test_search_with_every_token_row_as_a_hit_is_the_exhaustive_ranking():
    """k' >= T: every document with a row is a candidate of every query with a live token, so the result is the ranking of an
    exhaustive ops.maxsim_ragged over all documents.  Q 4 here (the first four tokens of every query: Q k' <= 16,384 hits
    with k' = 4,096 >= T = 4,071 rows)."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    c, ids, _, _, st = _exact()
    T, n = st.tokens.shape[0], len(ids)
    q = torch.from_numpy(c["q"][:, :4]).half().to(dev)
    assert T <= 4096 and bool((q != 0).any(-1).any(-1).all())
    s, d = st.search_device(q, n, 4096)
    b = torch.from_numpy(c["begin"]).to(dev).repeat(5)
    e = torch.from_numpy(c["end"]).to(dev).repeat(5)
    full = ops.maxsim_ragged(q, st.tokens, b, e, None, pairs_per_query=n, sim_round=True).view(5, n)
    order = torch.sort(full, dim=1, descending=True, stable=True)          # stable: equal scores, lower document first
    assert torch.equal(d, order.indices) and torch.equal(s, order.values)


def test_search_pads_with_minus_infinity_and_minus_one():
    dev = util.require_gpu()
    c, ids, _, _, st = _exact()
    q = torch.from_numpy(c["q"]).half().to(dev)
    q[2] = 0                                                               # a query whose tokens are all zero
    top_n = 150                                                            # more than the at most 6 x 16 candidates
    s, d = st.search_device(q, top_n, c["k"])
    ref_s, ref_d, cands = R.search_ref(q.float().cpu().numpy(), c["tokens"], c["begin"], c["end"], c["k"], top_n, sim_round=True)
    assert np.array_equal(d.cpu().numpy(), ref_d) and np.array_equal(s.cpu().numpy(), ref_s)
    assert 0 < max(len(x) for x in cands) < top_n and cands[2] == []
    assert bool((d[2] == -1).all()) and bool(torch.isinf(s[2]).all()) and bool((s[2] < 0).all())
    res = st.search(q, top_n, c["k"])
    assert res[2] == [] and [len(r) for r in res] == [len(x) for x in cands]


def test_round_trip_through_the_reference_layout(tmp_path):
    """write_reference_store -> TokenStore.load -> search: (seq_id, score) lists equal to the device result mapped on the host."""
    from matchmaker_amd.token_store import TokenStore, write_reference_store
    dev = util.require_gpu()
    c, ids, _, ref, _ = _exact()
    docs = [c["tokens"][b:e].astype(np.float16) for b, e in zip(c["begin"], c["end"])]
    write_reference_store(str(tmp_path), docs, ids, token_block_size=1500, token_dtype="float16")     # three files
    st = TokenStore.load(str(tmp_path), 128, "float16", 1500, dev)
    q = torch.from_numpy(c["q"]).half().to(dev)
    res = st.search(q, c["top_n"], c["k"])
    s, d = st.search_device(q, c["top_n"], c["k"])
    assert res == [[(ids[j], float(x)) for x, j in zip(si, di) if j >= 0] for si, di in zip(s.cpu().tolist(), d.cpu().tolist())]
    assert np.array_equal(d.cpu().numpy(), ref[True][1]) and np.array_equal(s.cpu().numpy(), ref[True][0])


def test_fp32_store_under_use_fp16_equals_the_fp16_store():
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    c, ids, _, ref, st16 = _exact()
    st32 = TokenStore(torch.from_numpy(c["tokens"]).to(dev), ids, c["begin"], c["end"])
    q = torch.from_numpy(c["q"]).to(dev)                                    # fp32 query vectors
    s32, d32 = st32.search_device(q, c["top_n"], c["k"], use_fp16=True)
    s16, d16 = st16.search_device(q, c["top_n"], c["k"], use_fp16=True)
    assert torch.equal(s32, s16) and torch.equal(d32, d16)
    assert np.array_equal(d32.cpu().numpy(), ref[True][1]) and np.array_equal(s32.cpu().numpy(), ref[True][0])


# ------------------------------------------------------------------------------------------ random-normal stores
@functools.lru_cache(maxsize=None)
def _normal(n_docs, seed):
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 71, n_docs)
    end = np.cumsum(lens).astype(np.int64)
    begin = end - lens
    tokens = torch.from_numpy(rng.standard_normal((int(end[-1]), 128)).astype(np.float32)).half()
    q = torch.from_numpy(rng.standard_normal((4, 32, 128)).astype(np.float32) / np.sqrt(128)).half()
    q[1, 20:] = 0
    st = TokenStore(tokens.to(dev), list(range(n_docs)), begin, end)
    return st, tokens, q, begin, end


def test_ivf_backed_token_search_with_every_list_probed_equals_the_flat_search():
    """200 documents, nlist 8, every list probed: the same token hits (random-normal rows: no equal scores for the two
    searches to order differently), so the same candidates and, from the same kernels, the same bits."""
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    dev = util.require_gpu()
    st, tokens, q, _, _ = _normal(200, 21)
    T = st.tokens.shape[0]
    ivf = IVFFlatIPIndexer({"token_dim": 128, "token_dtype": "float16", "faiss_ivf_list_count": 8,
                            "faiss_ivf_search_probe_count": 8}, device=dev)
    ivf.train_resident(st.tokens)
    ivf.index_resident(torch.arange(T, device=dev), st.tokens)
    flat_hits = st.token_hits(q.to(dev), 16)
    ivf_hits = st.token_hits(q.to(dev), 16, index=ivf)
    k_sorted = lambda h: torch.sort(h.view(-1, 16), dim=1).values       # the same rows per token (the two kernels may sum in another order)
    assert torch.equal(k_sorted(flat_hits), k_sorted(ivf_hits))
    s0, d0 = st.search_device(q.to(dev), 50, 16)
    s1, d1 = st.search_device(q.to(dev), 50, 16, index=ivf, query_chunk=40)
    assert torch.equal(s0, s1) and torch.equal(d0, d1) and bool((d0[:, 0] >= 0).all())


def test_random_normal_store_candidates_exact_and_scores_within_the_ragged_tolerance():
    """300 documents.  The candidates are checked against candidates_ref applied to the device's OWN token hits (exact; the
    token search's arithmetic is ops.dot_topk's tests' business); the scores against the fp64 MaxSim of those candidates under
    the tolerance the ragged MaxSim tests use for 16-bit stores (util.TOL_BF16 + 1e-4 |ref|, fp32 similarities)."""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    st, tokens, q, begin, end = _normal(300, 22)
    hits = st.token_hits(q.to(dev), 32)
    h = hits.cpu().numpy()
    assert (h[1].reshape(32, 32)[20:] == -1).all() and (h[0] >= 0).all()
    cands = R.candidates_ref_fast(h, begin, end)
    got = ops.colbert_candidates(hits, st._begin_sorted, st._end_sorted, st._doc_of_sorted, st.tokens.shape[0])
    for g, w in zip(got, R.padded_candidates(cands, begin, end, got[0].shape[1])):
        assert np.array_equal(g.cpu().numpy(), w)
    top_n = max(len(x) for x in cands)
    s, d = st.search_device(q.to(dev), top_n, 32, use_fp16=False)
    s, d = s.cpu().numpy(), d.cpu().numpy()
    q64, t64 = q.double().numpy(), tokens.double().numpy()
    for i in range(q.shape[0]):
        n = len(cands[i])
        assert sorted(d[i, :n].tolist()) == cands[i] and (d[i, n:] == -1).all() and (np.diff(s[i, :n]) <= 0).all()
        for sc, j in zip(s[i, :n], d[i, :n]):
            ref = float((q64[i] @ t64[begin[j]: end[j]].T).max(-1).sum())
            assert abs(sc - ref) <= util.TOL_BF16 + 1e-4 * abs(ref), (i, j, sc, ref)


def test_ranking_the_hits_replays_from_a_graph_bit_equal():
    """Steps 4-7 with trim=False (no read-back) captured into one graph: a single chain of four launches on the capturing
    stream, no parallel branches; the replay gives the eager result bit for bit."""
    dev = util.require_gpu()
    st, tokens, q, _, _ = _normal(300, 22)
    qd = q.to(dev)
    hits = st.token_hits(qd, 32)
    s_ref, d_ref = st.rank_hits(qd, hits, 40, trim=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                           # warm-up outside the capture
        st.rank_hits(qd, hits, 40, trim=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s_g, d_g = st.rank_hits(qd, hits, 40, trim=False)
    for _ in range(2):
        s_g.fill_(0)
        d_g.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_g, s_ref) and torch.equal(d_g, d_ref)
