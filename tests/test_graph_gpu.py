"""GPU tests of the graph index: the beam search (ops.graph_search = mm_graph_search_fwd), the device construction
(matchmaker_amd.retrieval.build_graph) and GraphIPIndexer against the numpy restatement in tests/graph_reference.py.
On the exact stores every inner product is exact in fp32 in any order, so rows, scores and stats must be EQUAL to the
restatement; the stores are full of equal scores, which pins the tie rule."""
import functools

import numpy as np
import pytest
import torch

from tests import graph_reference as GR
from tests import util

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _store(n, E, M):
    """(x float32 [n, E] of an exact store, its graph from the restatement); shared, never modified"""
    x = GR.exact_store(n, E, seed=n + E, dtype=np.float32)
    g = GR.build(x, M)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


def _queries(nq, E, seed):
    return GR.exact_store(nq, E, seed=seed, dtype=np.float32)


def _entries(nq, n, count, seed):
    return np.random.default_rng(seed).integers(0, n, (nq, count)).astype(np.int32)


def _run(dev, dtype, x, g, q, e, ef, k, width, max_iters=None):
    from matchmaker_amd import ops
    s, r, st = ops.graph_search(torch.from_numpy(q).to(dev).to(dtype), torch.from_numpy(x).to(dev).to(dtype),
                                torch.from_numpy(g).to(dev), torch.from_numpy(e).to(dev), ef, k, width, max_iters, return_stats=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy(), st.cpu().numpy()


def _assert_equal(got, ref, what=""):
    s, r, st = got
    rs, rr, it, sc = ref
    assert (r == rr).all(), (what, np.argwhere(r != rr)[:5])
    assert (s.astype(np.float64) == rs).all(), what
    assert (st[:, 0] == it).all() and (st[:, 1] == sc).all(), (what, st[:3], it[:3], sc[:3])


def _reachable(g, entries):
    seen = set(int(t) for t in entries if t >= 0)
    todo = list(seen)
    while todo:
        for nb in g[todo.pop()].tolist():
            if nb >= 0 and nb not in seen:
                seen.add(nb)
                todo.append(nb)
    return seen


CASES = [(1500, 128, 8, 32, 1, 10), (1500, 768, 16, 64, 4, 64), (3000, 384, 128, 128, 8, 100), (700, 256, 32, 700, 2, 700)]


@pytest.mark.parametrize("nq", [1, 37])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n,E,M,ef,width,k", CASES)
def test_search_is_bit_equal_to_the_restatement_on_exact_stores(n, E, M, ef, width, k, dtype, nq):
    dev = util.require_gpu()
    x, g = _store(n, E, M)
    q = _queries(nq, E, seed=1000 + nq)
    e = _entries(nq, n, min(ef, 8), seed=n + nq)
    mi = GR.default_max_iters(ef, width)
    ref = GR.search(x, g, q, e, ef, width, mi, k)
    got = _run(dev, dtype, x, g, q, e, ef, k, width)           # max_iters=None: the same default
    _assert_equal(got, ref, (n, E, M, ef, width, k, nq))
    if ef >= n:                                                 # every reachable row comes back
        for r in range(nq):
            reach = _reachable(g, e[r])
            assert set(got[1][r][got[1][r] >= 0].tolist()) == reach and ref[3][r] == len(reach)


def test_search_edge_cases_equal_the_restatement():
    dev = util.require_gpu()
    x, g = _store(1500, 128, 8)
    n, nq = x.shape[0], 5
    q = _queries(nq, 128, seed=77)
    # entry rows with -1 and duplicates (one query has no entry at all)
    e = _entries(nq, n, 8, seed=5)
    e[0, 1] = e[0, 0]
    e[0, 5] = e[0, 0]
    e[1, ::2] = -1
    e[2, :] = -1
    e[3, :] = e[3, 0]
    _assert_equal(_run(dev, torch.float16, x, g, q, e, 32, 10, 2), GR.search(x, g, q, e, 32, 2, 24, 10), "entries")
    # neighbour rows that are all -1: the entry rows of query 0 lead nowhere, a fifth of the other rows are dead ends
    g2 = g.copy()
    g2[np.random.default_rng(6).random(n) < 0.2] = -1
    g2[e[0][e[0] >= 0]] = -1
    ref = GR.search(x, g2, q, e, 32, 2, 24, 10)
    assert ref[2][0] >= 1 and ref[3][0] == len(set(e[0].tolist()))
    _assert_equal(_run(dev, torch.float16, x, g2, q, e, 32, 10, 2), ref, "dead ends")
    # k larger than the number of rows reached: -inf / -1 padding
    g3 = np.full_like(g, -1)
    ref = GR.search(x, g3, q, e, 32, 4, 16, 32)
    got = _run(dev, torch.bfloat16, x, g3, q, e, 32, 32, 4)
    _assert_equal(got, ref, "padding")
    d = len(set(e[0].tolist()))
    assert (got[1][0, d:] == -1).all() and np.isneginf(got[0][0, d:]).all() and (got[1][2] == -1).all()
    # one iteration only
    e4 = _entries(nq, n, 8, seed=8)
    ref = GR.search(x, g, q, e4, 32, 4, 1, 32)
    assert (ref[2] == 1).all()
    _assert_equal(_run(dev, torch.float16, x, g, q, e4, 32, 32, 4, max_iters=1), ref, "max_iters = 1")
    # as many entry rows as the list holds
    e5 = _entries(nq, n, 48, seed=9)
    _assert_equal(_run(dev, torch.float16, x, g, q, e5, 48, 48, 3), GR.search(x, g, q, e5, 48, 3, GR.default_max_iters(48, 3), 48),
                  "n_entry = ef")


def test_both_visited_table_placements_give_the_restatements_result():
    from matchmaker_amd import _lib
    dev = util.require_gpu()
    n, E, M, ef, width, k, nq = 3000, 384, 128, 32, 8, 32, 9
    x, g = _store(n, E, M)
    q = _queries(nq, E, seed=31)
    e = _entries(nq, n, 16, seed=32)
    L = _lib.lib()
    assert L.mm_graph_search_workspace_bytes(n, nq, M, ef, width, 16, 7) == 256              # 16 + 7 * 1024 rows: LDS
    assert L.mm_graph_search_workspace_bytes(n, nq, M, ef, width, 16, 512) == nq * 8192 * 4  # 16 + 512 * 1024: workspace
    ref = GR.search(x, g, q, e, ef, width, 512, k)
    assert ref[2].max() <= 7                                   # the list runs dry within 7 iterations: one result for both limits
    in_lds = _run(dev, torch.float16, x, g, q, e, ef, k, width, max_iters=7)
    in_ws = _run(dev, torch.float16, x, g, q, e, ef, k, width, max_iters=512)
    _assert_equal(in_lds, ref, "LDS")
    _assert_equal(in_ws, ref, "workspace")
    for a, b in zip(in_lds, in_ws):
        assert (a == b).all()
    # more queries than workgroups (1,024): a workgroup clears its table again for its next query; the queries of the second
    # pass against the restatement, each placement under its own iteration limit
    nq2 = 1100
    q2 = _queries(nq2, E, seed=33)
    e2 = np.repeat(e, -(-nq2 // nq), axis=0)[:nq2]
    for mi in (7, 512):
        got = _run(dev, torch.float16, x, g, q2, e2, ef, k, width, max_iters=mi)
        _assert_equal([t[1024:] for t in got], GR.search(x, g, q2[1024:], e2[1024:], ef, width, mi, k), f"second pass, max_iters {mi}")


@pytest.mark.parametrize("n,E,M", [(1200, 128, 8), (1200, 128, 128), (40, 128, 64)])
def test_device_construction_equals_the_restatement(n, E, M):
    from matchmaker_amd.retrieval import build_graph
    dev = util.require_gpu()
    x, ref = _store(n, E, M)
    got = build_graph(torch.from_numpy(x).to(dev).half(), M, block=512).cpu().numpy()       # several query blocks
    assert got.dtype == np.int32 and got.shape == (n, M)
    assert (got == ref).all(), np.argwhere(got != ref)[:5]
    for v in range(n):
        row = got[v][got[v] >= 0].tolist()
        assert v not in row and len(set(row)) == len(row)
        assert (got[v][len(row):] == -1).all()
    if n - 1 < M:
        assert (got[:, n - 1:] == -1).all() and (got[:, : n - 1] >= 0).all()


@pytest.fixture(scope="module")
def recall_index():
    """the recall collection, indexed on the device; ids = 7 row + 3"""
    from matchmaker_amd.retrieval import GraphIPIndexer
    dev = util.require_gpu()
    x, q = GR.recall_collection()
    ix = GraphIPIndexer({"token_dim": 128, "faiss_hnsw_graph_neighbors": 16, "faiss_hnsw_efSearch": 64, "faiss_hnsw_efConstruction": 40,
                         "graph_entry_sample": 256, "graph_entry_count": 16}, device=dev)
    ix.index([np.arange(x.shape[0], dtype=np.int64) * 7 + 3], [x])
    xf, qf = x.astype(np.float64), q.astype(np.float64)
    _, truth = GR.topk_ip(qf, xf, 10)
    return ix, xf, qf, q, truth


@pytest.mark.parametrize("width", [1, 4])
def test_real_valued_collection_scores_order_and_recall(recall_index, width):
    from matchmaker_amd import ops
    ix, xf, qf, q, truth = recall_index
    n, E = xf.shape
    qd = torch.from_numpy(q).to(ix.device)
    entry = ix.entry_rows(qd, 64)
    assert entry.shape == (q.shape[0], 16) and entry.dtype == torch.int32
    assert np.isin(entry.cpu().numpy(), GR.sample_rows(n, 256)).all()
    s, rows = ops.graph_search(qd, ix.vectors, ix.neighbors, entry, 64, 64, width)
    s, rows = s.cpu().numpy().astype(np.float64), rows.cpu().numpy()
    recalls = []
    for r in range(q.shape[0]):
        got = rows[r]
        assert (got >= 0).all() and (got < n).all() and len(set(got.tolist())) == got.size, r
        assert (np.diff(s[r]) <= 0).all(), r
        tie = np.diff(s[r]) == 0
        assert (np.diff(got)[tie] > 0).all(), r                # equal scores: lower row first
        exact = xf[got] @ qf[r]
        bound = (E - 1) * 2.0 ** -24 * (np.abs(xf[got]) @ np.abs(qf[r]))     # an fp32 sum of exact products, any order
        assert (np.abs(s[r] - exact) <= bound).all(), (r, np.abs(s[r] - exact).max(), bound.min())
        recalls.append(len(set(got[:10].tolist()) & set(truth[r].tolist())) / 10)
    print(f"width {width}: mean recall@10 {np.mean(recalls):.4f}, worst query {min(recalls):.2f}")
    assert np.mean(recalls) >= 0.95


def test_envelope_is_refused_as_unsupported():
    from matchmaker_amd import ops, _lib, NativeError
    dev = util.require_gpu()
    q = torch.zeros(2, 128, dtype=torch.float16, device=dev)
    v = torch.zeros(50, 128, dtype=torch.float16, device=dev)
    g = torch.full((50, 8), -1, dtype=torch.int32, device=dev)
    e = torch.zeros(2, 4, dtype=torch.int32, device=dev)
    for what, args in (("ef = 4096", (q, v, g, e, 4096, 10)), ("odd M", (q, v, g[:, :7], e, 16, 10)), ("k > ef", (q, v, g, e, 16, 17))):
        with pytest.raises(NativeError) as err:
            ops.graph_search(*args)
        assert err.value.code == _lib.MM_EUNSUPPORTED, what
    # the same four through the raw ABI, E = 96 unpadded, on sentinel-filled outputs: nothing is launched
    s = torch.full((2, 10), 5.0, dtype=torch.float32, device=dev)
    r = torch.full((2, 10), 5, dtype=torch.int64, device=dev)
    st = torch.full((2, 2), 5, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=dev)
    ok = dict(E=128, M=8, ef=16, k=10)
    for what, bad in (("96", dict(E=96)), ("4096", dict(ef=4096)), ("M=7", dict(M=7)), ("k=17", dict(k=17))):
        a = dict(ok, **bad)
        rc = _lib.lib().mm_graph_search_fwd(q.data_ptr(), v.data_ptr(), g.data_ptr(), e.data_ptr(), 50, 2, a["E"], _lib.MM_F16, a["M"], 4,
                                            a["ef"], 2, 8, a["k"], s.data_ptr(), r.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.MM_EUNSUPPORTED, what
        with pytest.raises(NativeError) as err:
            _lib.check(rc, "mm_graph_search_fwd")
        assert err.value.code == _lib.MM_EUNSUPPORTED and what in str(err.value)
        torch.cuda.synchronize()
        assert (s == 5.0).all() and (r == 5).all() and (st == 5).all(), what
    s2, r2 = ops.graph_search(q[:, :96], v[:, :96], g, e, 16, 10)          # ops pads instead
    assert s2.shape == (2, 10) and (r2[:, 0] == 0).all() and (r2[:, 1:] == -1).all()


def test_indexer_end_to_end_with_external_ids(recall_index):
    from matchmaker_amd import ops
    ix, xf, qf, q, truth = recall_index
    qd = torch.from_numpy(q).to(ix.device)
    for top_n, ef in ((10, 64), (100, 100)):                   # top_n > efSearch widens ef
        s, ids = ix.search(q.astype(np.float32), top_n)
        rs, rr = ops.graph_search(qd, ix.vectors, ix.neighbors, ix.entry_rows(qd, ef), ef, top_n, 4)
        rs, rr = rs.cpu().numpy(), rr.cpu().numpy()
        assert s.shape == (q.shape[0], top_n) and ids.dtype == np.int64
        assert (s == rs).all() and (ids == np.where(rr >= 0, rr * 7 + 3, -1)).all()
        assert (rr >= 0).all()
    s1, i1 = ix.search(q[0].astype(np.float32), 5)             # a 1-d query
    assert s1.shape == (1, 5) and (i1[0] == ix.search(q.astype(np.float32), 5)[1][0]).all()
