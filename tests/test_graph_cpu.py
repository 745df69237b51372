"""CPU tests of the graph index (matchmaker_amd.retrieval.GraphIPIndexer, mm_graph_search_fwd): the C ABI and its binding,
the fake-tensor rule, the indexer's host logic with the numpy restatement (tests/graph_reference.py) standing in for the
device operators, and the restatement's own recall."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import graph_reference as GR

SYMBOLS = ("mm_graph_search_workspace_bytes", "mm_graph_search_fwd")


def _indexer(E, M=8, ef=16, **cfg):
    from matchmaker_amd.retrieval import GraphIPIndexer
    c = {"token_dim": E, "faiss_hnsw_graph_neighbors": M, "faiss_hnsw_efSearch": ef, "faiss_hnsw_efConstruction": 128}
    c.update(cfg)
    return GraphIPIndexer(c, device="cpu", topk_fn=GR.topk_fn, search_fn=GR.search_fn, merge_fn=GR.merge_fn)


def _data(n=300, E=40, seed=3):
    x = np.random.default_rng(seed).standard_normal((n, E)).astype(np.float32)
    chunks = [x[: n // 3], x[n // 3:]]
    ids = [np.arange(0, n // 3, dtype=np.int64) * 3 + 5, np.arange(n // 3, n, dtype=np.int64) * 3 + 5]
    return x, chunks, ids


def _padded16(a, E_pad=128):
    out = np.zeros((a.shape[0], E_pad), np.float32)
    out[:, : a.shape[1]] = a.astype(np.float16)
    return out


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays_4():
    from matchmaker_amd import build, _lib
    from tests import abi
    L = abi.assert_bound(SYMBOLS)
    assert "graph_search.hip" in build.SOURCES
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    # the visited table fits LDS: a token workspace; it does not: one slice per workgroup, never more than 1024 of them
    assert L.mm_graph_search_workspace_bytes(3000, 37, 16, 64, 4, 16, 24) == 256
    big = L.mm_graph_search_workspace_bytes(3000, 37, 128, 128, 8, 16, 512)
    assert big == 37 * 8192 * 4                        # 2 min(n, bound) = 6000 slots -> 8192
    assert L.mm_graph_search_workspace_bytes(3000, 5000, 128, 128, 8, 16, 512) == 1024 * 8192 * 4
    assert L.mm_graph_search_workspace_bytes(3000, 37, 15, 64, 4, 16, 24) == 0          # outside the envelope
    # the largest table of the envelope: 2 (2048 + 65536 * 8 * 128) slots -> 2^28 of them, 4 bytes each, per workgroup
    assert L.mm_graph_search_workspace_bytes((1 << 31) - 1, 3, 128, 2048, 8, 2048, 65536) == 3 * (1 << 28) * 4
    # refused before anything touches the device
    buf = (torch.zeros(1 << 12, dtype=torch.float32)).data_ptr()
    ok = dict(n=100, nq=1, E=128, dtype=_lib.MM_F16, M=8, n_entry=4, ef=16, width=2, max_iters=4, k=8)

    def call(ws_bytes=1 << 12, **kw):
        a = dict(ok, **kw)
        return L.mm_graph_search_fwd(buf, buf, buf, buf, a["n"], a["nq"], a["E"], a["dtype"], a["M"], a["n_entry"], a["ef"],
                                     a["width"], a["max_iters"], a["k"], buf, buf, None, buf, ws_bytes, None)

    for bad in (dict(E=96), dict(E=896), dict(ef=4096), dict(ef=0), dict(M=7), dict(M=130), dict(k=17), dict(k=0), dict(width=9),
                dict(width=0), dict(n_entry=17), dict(n_entry=0), dict(dtype=_lib.MM_F32), dict(n=1 << 31), dict(max_iters=0),
                dict(max_iters=65537)):
        assert call(**bad) == _lib.MM_EUNSUPPORTED, bad
    assert L.mm_last_error()
    assert call(ws_bytes=16) == _lib.MM_EWORKSPACE
    assert L.mm_graph_search_fwd(None, buf, buf, buf, 100, 1, 128, _lib.MM_F16, 8, 4, 16, 2, 4, 8, buf, buf, None, buf, 1 << 12,
                                 None) == _lib.MM_EINVAL


def test_fake_tensor_rule_and_argument_checks():
    from matchmaker_amd import ops, NativeError, torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        q, v = torch.empty(5, 256, dtype=torch.float16, device="cuda"), torch.empty(90, 256, dtype=torch.float16, device="cuda")
        g, e = torch.empty(90, 16, dtype=torch.int32, device="cuda"), torch.empty(5, 4, dtype=torch.int32, device="cuda")
        s, r, st = torch.ops.mm_native.graph_search(q, v, g, e, 32, 10)
        assert s.shape == (5, 10) and s.dtype == torch.float32 and s.device.type == "cuda"
        assert r.shape == (5, 10) and r.dtype == torch.int64
        assert st.shape == (5, 2) and st.dtype == torch.int32
        s, r, st = torch.ops.mm_native.graph_search(q, v, g, e, 32, 32, 8, 3)
        assert s.shape == (5, 32) and r.shape == (5, 32)
    assert len(torch.ops.mm_native.graph_search.default._schema.arguments) == 8
    m = dict(device="meta")
    q, v = torch.empty(5, 256, dtype=torch.float16, **m), torch.empty(90, 256, dtype=torch.float16, **m)
    g, e = torch.empty(90, 16, dtype=torch.int32, **m), torch.empty(5, 4, dtype=torch.int32, **m)
    with pytest.raises(NativeError, match="CPU"):
        ops.graph_search(torch.zeros(1, 128, dtype=torch.float16), torch.zeros(4, 128, dtype=torch.float16),
                         torch.zeros(4, 2, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), 4, 2)
    for args in [(q.float(), v.float(), g, e, 32, 10), (q, v[:, :128], g, e, 32, 10), (q, v, g.long(), e, 32, 10),
                 (q, v, g[:50], e, 32, 10), (q, v, g, e.long(), 32, 10), (q, v, g, e[:3], 32, 10)]:
        with pytest.raises(NativeError):
            ops.graph_search(*args)


def test_construction_restatement_on_a_hand_checked_store():
    """5 rows on a line: the inner product orders rows by their coordinate, so every list can be written down."""
    x = np.zeros((5, 128))
    x[:, 0] = [1, 2, 3, 4, 5]
    knn = GR.knn_lists(x, 2)
    # top 3 of row v by score x_u x_v: rows 4, 3, 2; v itself leaves when it is among them, else the last entry does
    assert knn.tolist() == [[4, 3], [4, 3], [4, 3], [4, 2], [3, 2]]
    g = GR.build(x, 2)
    # fwd = [4], [4], [4], [4], [3]; reverse edges: row 4 gets 0 (then full), row 3 gets 4; the rest fill from knn
    assert g.tolist() == [[4, 3], [4, 3], [4, 3], [4, 2], [3, 0]]
    small = GR.build(x[:3], 4)                                # N - 1 < M: -1 padded
    assert small.shape == (3, 4) and (small[:, 2:] == -1).all() and (small[:, :2] >= 0).all()


def test_device_construction_path_equals_the_restatement_on_the_cpu():
    """build_graph's sorted torch ops, run on CPU tensors with the restatement's top-k standing in"""
    from matchmaker_amd.retrieval import build_graph
    for n, M in ((150, 8), (20, 32), (64, 2)):
        x = GR.exact_store(n, 128, seed=n + M, dtype=np.float32)
        got = build_graph(torch.from_numpy(x).half(), M, GR.topk_fn, block=64)
        ref = GR.build(x, M)
        assert got.dtype == torch.int32 and (got.numpy() == ref).all(), (n, M)
        for v in range(n):
            row = [t for t in ref[v].tolist() if t >= 0]
            assert v not in row and len(set(row)) == len(row)


def test_construction_ranks_rows_the_topk_operator_cannot_decide_in_full():
    """a top-k operator that gives up on any call holding one of three rows (what ops.dot_topk does for a query its
    threshold protocol cannot decide): the blocks are halved down to those rows, which are ranked in full — same graph"""
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import build_graph, _knn_block
    n, M = 300, 8
    x = GR.exact_store(n, 128, seed=11, dtype=np.float32)           # full of equal scores: the tie rule of the fallback
    xt = torch.from_numpy(x).half()
    bad = (0, 137, 299)
    calls = []

    def stubborn(q, c, k):
        lo = next(i for i in range(n - q.shape[0] + 1) if torch.equal(c[i: i + q.shape[0]], q))
        calls.append((lo, lo + q.shape[0]))
        if any(lo <= r < lo + q.shape[0] for r in bad):
            raise NativeError("dot_topk: 1 queries without an exact top-k", -4)
        return GR.topk_fn(q, c, k)

    got = build_graph(xt, M, stubborn, block=128)
    assert (got.numpy() == GR.build(x, M)).all()
    assert any(hi - lo <= 16 for lo, hi in calls) and sum(1 for lo, hi in calls if any(lo <= r < hi for r in bad)) >= 3
    idx = _knn_block(xt[:40], 0, 40, 64, lambda q, c, k: (_ for _ in ()).throw(NativeError("never decides")))
    assert idx.shape == (40, 64) and (idx[:, 40:] == -1).all()      # fewer rows than k: -1 padded, like the operator
    assert (idx.numpy() == GR.topk_ip(x[:40], x[:40], 64)[1]).all()


def test_search_restatement_edge_cases():
    x = GR.exact_store(60, 128, seed=1, dtype=np.float32)
    g = GR.build(x, 4)
    q = GR.exact_store(2, 128, seed=2, dtype=np.float32)
    e = np.array([[3, -1, 3, 7], [-1, -1, -1, -1]], np.int32)
    s, r, it, sc = GR.search(x, g, q, e, ef=8, width=2, max_iters=1, k=8)
    assert it.tolist() == [1, 0] and sc[1] == 0 and (r[1] == -1).all() and np.isneginf(s[1]).all()
    assert 2 <= sc[0] <= 2 + 2 * 4                            # the two distinct entries + at most two rows of neighbours
    full = np.asarray(x, np.float64) @ np.asarray(q[0], np.float64)
    kk = int((r[0] >= 0).sum())
    assert (s[0, :kk] == full[r[0, :kk]]).all() and (np.diff(s[0, :kk]) <= 0).all()


def test_indexer_ids_ef_and_search_against_the_restatement():
    x, chunks, ids = _data()
    ix = _indexer(x.shape[1], M=8, ef=16, graph_entry_sample=64, graph_entry_count=6, graph_search_width=2)
    ix.prepare(chunks)
    ix.index(ids, chunks)
    n = x.shape[0]
    xp = _padded16(x)
    assert ix.vectors.shape == (n, 128) and (ix.vectors.float().numpy() == xp).all()
    assert (ix.ids.numpy() == np.concatenate(ids)).all()
    assert (ix.neighbors.numpy() == GR.build(xp, 8)).all()
    assert (ix.sample_rows.numpy() == GR.sample_rows(n, 64)).all()
    assert ix.sample_vectors.is_contiguous() and (ix.sample_vectors.float().numpy() == xp[GR.sample_rows(n, 64)]).all()
    qv = np.random.default_rng(9).standard_normal((5, x.shape[1])).astype(np.float32)
    q16 = _padded16(qv)
    for top_n, ef in ((10, 16), (40, 40)):                     # ef = max(efSearch, top_n)
        s, i = ix.search(qv, top_n)
        entry = GR.entries_from_sample(xp, q16, GR.sample_rows(n, 64), 6)
        rs, rr, _, _ = GR.search(xp, ix.neighbors.numpy(), q16, entry, ef, 2, GR.default_max_iters(ef, 2), top_n)
        assert s.shape == (5, top_n) and i.dtype == np.int64
        np.testing.assert_allclose(s, rs, atol=1e-6)
        assert (i == np.where(rr >= 0, np.concatenate(ids)[np.maximum(rr, 0)], -1)).all()
    seen = {}
    ix._search = lambda q, v, g, e, ef, k, width: seen.update(ef=ef, k=k, width=width, n_entry=e.shape[1]) or GR.search_fn(q, v, g, e, ef, k, width)
    ix.search(qv[0], 3)                                        # a 1-d query
    assert seen == dict(ef=16, k=3, width=2, n_entry=6)
    ix.search(qv, 50)
    assert seen["ef"] == 50 and seen["k"] == 50
    ix.entry_count = 100
    ix.search(qv, 4)
    assert seen["n_entry"] == 16                               # min(entry count, ef, S)


def test_save_load_round_trip_and_foreign_files(tmp_path):
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    ix = _indexer(x.shape[1], graph_entry_sample=50)
    ix.index(ids, chunks)
    qv = np.random.default_rng(3).standard_normal((4, x.shape[1])).astype(np.float32)
    s0, i0 = ix.search(qv, 10)
    path = str(tmp_path / "graph.index")
    ix.save(path)
    ix2 = _indexer(x.shape[1], graph_entry_sample=50)
    ix2.load(path)
    assert torch.equal(ix2.neighbors, ix.neighbors) and torch.equal(ix2.sample_rows, ix.sample_rows)
    assert torch.equal(ix2.sample_vectors, ix.sample_vectors) and torch.equal(ix2.ids, ix.ids)
    s1, i1 = ix2.search(qv, 10)
    assert (s0 == s1).all() and (i0 == i1).all()
    ix3 = _indexer(x.shape[1])
    ix3.load(path, config_overwrites={"faiss_hnsw_efSearch": 77})
    assert ix3.ef_search == 77
    bogus = tmp_path / "faiss.index"
    bogus.write_bytes(b"IxMp" + bytes(64))                     # what faiss.write_index starts an IndexIDMap file with
    with pytest.raises(NativeError, match="faiss"):
        _indexer(x.shape[1]).load(str(bogus))
    other = tmp_path / "other.npz"
    with open(other, "wb") as f:
        np.savez(f, magic=np.array("matchmaker_amd.IVFFlatIPIndexer"), format=np.array(1))
    with pytest.raises(NativeError, match="GraphIPIndexer file"):
        _indexer(x.shape[1]).load(str(other))
    with pytest.raises(NativeError, match="-dim"):
        _indexer(x.shape[1] + 1).load(path)
    # the file decides what was built, the config how it is searched
    ix4 = _indexer(x.shape[1], M=4, ef=33, graph_entry_sample=7, graph_entry_count=3, graph_search_width=1)
    ix4.load(path)
    assert (ix4.M, ix4.entry_sample, ix4.ef_search, ix4.entry_count, ix4.width) == (8, 50, 33, 3, 1)
    # damaged archives never reach the search
    z = dict(np.load(path, allow_pickle=False))
    for damage in (dict(neighbors=z["neighbors"][:-1]), dict(neighbors=z["neighbors"][:, :6]), dict(ids=z["ids"][:-1]),
                   dict(sample_rows=np.array([0, 300])), dict(neighbors=np.where(z["neighbors"] == 5, 300, z["neighbors"])),
                   dict(M=np.array(6))):
        broken = tmp_path / "broken.npz"
        with open(broken, "wb") as f:
            np.savez(f, **dict(z, **damage))
        with pytest.raises(NativeError, match="damaged"):
            _indexer(x.shape[1]).load(str(broken))


def test_refuses_fp32_stores_and_bad_configs():
    from matchmaker_amd import NativeError, GraphIPIndexer
    with pytest.raises(NativeError, match="float16"):
        GraphIPIndexer({"token_dim": 40, "token_dtype": "float32", "faiss_hnsw_graph_neighbors": 8, "faiss_hnsw_efSearch": 16},
                       device="cpu")
    for bad in (dict(M=7), dict(M=130), dict(ef=0), dict(graph_search_width=9)):
        with pytest.raises(NativeError):
            _indexer(40, **bad)
    with pytest.raises(NativeError, match="index"):
        _indexer(40).search(np.zeros(40, np.float32), 3)


# ---- sharded graph index under gloo ------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


N_SHARDED = 121                                                # odd: uneven shards


def _exhaustive_indexer(E):
    """every shard is searched exhaustively: all of its rows are entry rows and ef covers them"""
    return _indexer(E, M=4, ef=N_SHARDED, graph_entry_sample=N_SHARDED, graph_entry_count=N_SHARDED)


def _graph_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from matchmaker_amd.sharding import shard_range
    x, chunks, ids = _data(n=N_SHARDED)
    ix = _exhaustive_indexer(x.shape[1])
    ix.index(ids, chunks)
    lo, hi = shard_range(N_SHARDED, world, rank)
    assert ix.vectors.shape == (hi - lo, 128) and ix.ids.tolist() == np.concatenate(ids)[lo:hi].tolist()
    assert (ix.neighbors.numpy() == GR.build(_padded16(x)[lo:hi], 4)).all()          # a graph of its own per shard
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    ix.save(os.path.join(out_dir, "graph.index"))
    np.save(os.path.join(out_dir, f"s{rank}.npy"), s)
    np.save(os.path.join(out_dir, f"i{rank}.npy"), i)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_sharded_graph_equals_single_process(tmp_path):
    world = 2
    mp.spawn(_graph_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert (np.load(tmp_path / "i0.npy") == np.load(tmp_path / "i1.npy")).all()
    assert os.path.exists(tmp_path / "graph.index.rank0") and os.path.exists(tmp_path / "graph.index.rank1")
    x, chunks, ids = _data(n=N_SHARDED)
    ix = _exhaustive_indexer(x.shape[1])
    ix.index(ids, chunks)
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    flat_s, flat_i = GR.topk_ip(_padded16(qv), _padded16(x), 25)
    np.testing.assert_allclose(s, flat_s, atol=1e-6)           # exhaustive: the single-shard result is the exact top-25
    assert (i == np.concatenate(ids)[flat_i]).all()
    np.testing.assert_allclose(np.load(tmp_path / "s0.npy"), s, atol=1e-6)
    assert (np.load(tmp_path / "i0.npy") == i).all()           # Gaussian scores: no ties to order differently


# ---- the restatement's own recall ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def recall_problem():
    x, q = GR.recall_collection()
    xf = x.astype(np.float64)
    g = GR.build(xf, 16)
    entry = GR.entries_from_sample(xf, q, GR.sample_rows(x.shape[0], 256), 16)
    _, truth = GR.topk_ip(q, xf, 10)
    return xf, q, g, entry, truth


@pytest.mark.parametrize("width", [1, 4])
def test_restatement_recall_on_the_recall_collection(recall_problem, width):
    """N 4096, E 128, M 16, ef 64, 16 entries from a 256-row stride sample, 64 queries: mean recall@10 >= 0.98 against the
    exhaustive float64 top-10"""
    x, q, g, entry, truth = recall_problem
    _, rows, iters, scored = GR.search(x, g, q, entry, 64, width, GR.default_max_iters(64, width), 10)
    per_query = [len(set(rows[r].tolist()) & set(truth[r].tolist())) / 10 for r in range(q.shape[0])]
    print(f"width {width}: mean recall@10 {np.mean(per_query):.4f}, worst query {min(per_query):.2f}, "
          f"mean iterations {iters.mean():.1f}, mean rows scored {scored.mean():.0f}")
    assert np.mean(per_query) >= 0.98
