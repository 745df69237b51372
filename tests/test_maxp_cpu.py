"""CPU: MaxP retrieval (retrieval.MaxPIndexer over ops.distinct_hits) — the reference restatement against
hand-written cases, the indexer's logic (widening, the cap, refusals, index_store) with numpy stand-ins for the two native
operators, the two-rank path under gloo, and the operator's registration."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from matchmaker_amd import NativeError, build, ops
from matchmaker_amd.retrieval import FlatIPIndexer, MaxPIndexer
from matchmaker_amd.token_store import TokenStore
from tests import abi
from tests import maxp_reference as R

NEG = -np.inf
I64_MAX = np.iinfo(np.int64).max


def test_the_translation_unit_is_built_and_bound():
    assert "distinct_hits.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "distinct_hits.hip"))
    abi.assert_bound(("mm_distinct_hits_fwd",))
    assert ops.DISTINCT_MAX_HITS == 8192 == MaxPIndexer.MAX_HITS


# ---- the reference restatement -----------------------------------------------------------------------------------------
def test_reference_on_hand_written_cases():
    ids = np.array([[7, 7, 3, -1, 3, 9, 7, 2],            # repeats, a dropped slot in the middle
                    [-1, -5, -1, -1, -1, -1, -1, -1],     # no valid hit; -5 is "no hit" too
                    [4, 4, 4, 4, 4, 4, 4, 4],             # one document
                    [I64_MAX, 0, I64_MAX, 1 << 40, (1 << 40) + 1, 1 << 41, 0, -1]], dtype=np.int64)
    sc = np.array([[9, 8, 7, 6, 5, 4, 3, 2], [1, 1, 1, 1, 1, 1, 1, 1], [5, 5, 5, 5, 5, 5, 5, 5],
                   [3, 3, 3, np.nan, -0.0, NEG, 9, 1]], dtype=np.float32)
    s, i, p, nd, nv = R.distinct_hits(sc, ids, 3)
    assert i.tolist() == [[7, 3, 9], [-1, -1, -1], [4, -1, -1], [I64_MAX, 0, 1 << 40]]
    assert p.tolist() == [[0, 2, 5], [-1, -1, -1], [0, -1, -1], [0, 1, 3]]
    assert nd.tolist() == [4, 0, 1, 5] and nv.tolist() == [7, 0, 8, 7]
    assert s[0].tolist() == [9, 7, 4] and s[1].tolist() == [NEG] * 3 and s[2].tolist() == [5, NEG, NEG]
    assert s[3, 0] == 3 and s[3, 1] == 3 and np.isnan(s[3, 2])               # scores are payload: the NaN is copied
    s, i, p, nd, nv = R.distinct_hits(sc, ids, 8)                            # top_n = K: everything, then the fill
    assert i[0].tolist() == [7, 3, 9, 2, -1, -1, -1, -1] and p[0].tolist() == [0, 2, 5, 7, -1, -1, -1, -1]
    assert i[3].tolist() == [I64_MAX, 0, 1 << 40, (1 << 40) + 1, 1 << 41, -1, -1, -1]
    assert np.signbit(s[3, 3]) and s[3, 3] == 0 and s[3, 4] == NEG and p[3, 4] == 5   # -0.0 and a real -inf hit are kept
    # an unsorted list: first occurrences in LIST order, not the maxima
    s, i, p, nd, nv = R.distinct_hits(np.array([[1, 9, 5, 7]], dtype=np.float32), np.array([[2, 2, 6, 6]], dtype=np.int64), 2)
    assert s.tolist() == [[1, 5]] and i.tolist() == [[2, 6]] and p.tolist() == [[0, 2]]


def test_brute_force_takes_every_documents_best_passage_lower_row_first():
    v = np.array([[1, 0], [3, 0], [2, 0], [3, 0], [0, 1]], dtype=np.float32)
    ids = np.array([10, 11, 10, 12, 13], dtype=np.int64)
    s, i, p, nd, nv = R.brute_force(np.array([[1, 0]], dtype=np.float32), v, ids, 3)
    assert i.tolist() == [[11, 12, 10]] and s.tolist() == [[3, 3, 2]] and nd.tolist() == [4] and nv.tolist() == [5]


# ---- the indexer over stand-ins ----------------------------------------------------------------------------------------------
def _topk_fn(calls=None):
    def fn(q, c, k):                                            # stand-in for ops.dot_topk: rows, lower row first on ties
        if calls is not None:
            calls.append((q.shape[0], k))
        s, _, rows = R.topk_hits(q.float().numpy(), c.float().numpy(), np.arange(c.shape[0]), k)
        return torch.from_numpy(s), torch.from_numpy(rows)
    return fn


def _distinct_fn(s, i, top_n):                                  # stand-in for ops.distinct_hits
    return tuple(torch.from_numpy(a) for a in R.distinct_hits(s.numpy(), i.numpy(), top_n))


def _merge_fn(s, ids, k):                                       # stand-in for ops.topk_merge
    s = s.clone()
    s[ids < 0] = float("-inf")
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), torch.gather(ids, 1, order)


E = 8


def _collection():
    """Document 0: 20 passages scoring 3 for query e0; documents 1..9: one passage scoring 2 for it; documents 10..14: one
    passage scoring 1..5 for query e1.  External id = 7 * document + 3."""
    vec, doc = [], []
    for _ in range(20):
        vec.append(3 * np.eye(E)[0]); doc.append(0)
    for d in range(1, 10):
        vec.append(2 * np.eye(E)[0]); doc.append(d)
    for d in range(10, 15):
        vec.append((d - 9) * np.eye(E)[1]); doc.append(d)
    return np.array(vec, dtype=np.float16), np.array(doc, dtype=np.int64) * 7 + 3


def _indexer(calls=None):
    vec, ids = _collection()
    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device="cpu", topk_fn=_topk_fn(calls), merge_fn=_merge_fn),
                     distinct_fn=_distinct_fn)
    ix.prepare([vec])
    ix.index([ids], [vec])
    return ix, vec, ids


QUERIES = np.eye(E, dtype=np.float32)[:2]


def test_one_search_without_widening_is_the_references_loop():
    calls = []
    ix, vec, ids = _indexer(calls)
    s, i, info = ix.search_device(QUERIES, 3, index_hit_top_n=4, return_info=True)
    assert calls == [(2, 4)]
    assert i.tolist() == [[3, -1, -1], [14 * 7 + 3, 13 * 7 + 3, 12 * 7 + 3]]
    assert s.tolist() == [[3, NEG, NEG], [5, 4, 3]]
    assert info["complete"].tolist() == [False, True] and info["n_distinct"].tolist() == [1, 4]
    assert info["pos"].tolist() == [[0, -1, -1], [0, 1, 2]] and info["hits_used"].tolist() == [4, 4]
    plain = ix.search_device(QUERIES, 3, index_hit_top_n=4)
    assert len(plain) == 2 and torch.equal(plain[1], i)
    # index_hit_top_n defaults to top_n (test_config.get("index_hit_top_n", top_n))
    del calls[:]
    ix.search_device(QUERIES, 3)
    assert calls == [(2, 3)]
    hs, hi = ix.search(QUERIES, 3, index_hit_top_n=4)
    assert isinstance(hs, np.ndarray) and hi.tolist() == i.tolist()


def test_widening_searches_only_the_incomplete_queries_again():
    calls = []
    ix, vec, ids = _indexer(calls)
    s, i, info = ix.search_device(QUERIES, 3, index_hit_top_n=4, widen=True, return_info=True)
    assert calls == [(2, 4), (1, 8), (1, 16), (1, 32)], calls                 # query 1 was complete after the first search
    assert info["complete"].tolist() == [True, True] and info["hits_used"].tolist() == [32, 4]
    assert i.tolist() == [[3, 10, 17], [14 * 7 + 3, 13 * 7 + 3, 12 * 7 + 3]] and s.tolist() == [[3, 2, 2], [5, 4, 3]]
    assert info["pos"].tolist() == [[0, 20, 21], [0, 1, 2]]
    # the same rows as ONE search with the final K, and as the brute force over all passages
    s1, i1 = ix.search_device(QUERIES, 3, index_hit_top_n=32)
    assert torch.equal(s1, s) and torch.equal(i1, i)
    bs, bi, _, _, _ = R.brute_force(QUERIES, vec, ids, 3)
    assert np.array_equal(bi, i.numpy()) and np.array_equal(bs.view(np.int32), s.numpy().view(np.int32))


def test_widening_stops_at_the_cap_and_leaves_the_row_flagged():
    calls = []
    vec = np.ones((9000, E), dtype=np.float16)                                 # one document of 9,000 passages
    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device="cpu", topk_fn=_topk_fn(calls)), distinct_fn=_distinct_fn)
    ix.index([np.full(9000, 5, dtype=np.int64)], [vec])
    s, i, info = ix.search_device(np.ones((1, E), dtype=np.float32), 2, widen=True, return_info=True)
    assert [k for _, k in calls] == [2 << j for j in range(13)] and calls[-1] == (1, 8192)
    assert info["complete"].tolist() == [False] and info["hits_used"].tolist() == [8192] and info["n_distinct"].tolist() == [1]
    assert i.tolist() == [[5, -1]] and s.tolist() == [[E, NEG]]
    # a lower cap of the caller's (the inner index's own k limit)
    del calls[:]
    ix = MaxPIndexer(ix.inner, distinct_fn=_distinct_fn, max_hits=48)
    _, _, info = ix.search_device(np.ones((1, E), dtype=np.float32), 2, index_hit_top_n=10, widen=True, return_info=True)
    assert [k for _, k in calls] == [10, 20, 40, 48] and info["hits_used"].tolist() == [48] and not info["complete"].any()
    with pytest.raises(NativeError, match="max_hits"):
        MaxPIndexer(ix.inner, max_hits=8193)


def test_an_exhausted_index_is_complete():
    ix, vec, ids = _indexer()
    s, i, info = ix.search_device(QUERIES[:1], 20, index_hit_top_n=64, return_info=True)      # 34 passages, 15 documents
    assert info["complete"].tolist() == [True] and info["n_distinct"].tolist() == [15]
    assert (i[0, 15:] == -1).all() and (i[0, :15] >= 0).all()


def test_refusals():
    ix, vec, ids = _indexer()
    for kw in (dict(top_n=8193), dict(top_n=10, index_hit_top_n=8193)):
        with pytest.raises(NativeError, match="8192") as e:
            ix.search_device(QUERIES, **kw)
        assert e.value.code == ops._lib.MM_EUNSUPPORTED
    with pytest.raises(NativeError, match="outside"):
        ix.search_device(QUERIES, 5, index_hit_top_n=4)
    with pytest.raises(NativeError, match="outside"):
        ix.search_device(QUERIES, 0)
    fp8_only = TokenStore(None, ["a", "b"], np.array([0, 2]), np.array([2, 3]), codes=torch.zeros(3, E, dtype=torch.uint8),
                          scales=torch.ones(3))
    with pytest.raises(NativeError, match="IVFFp8IPIndexer"):
        ix.index_store(fp8_only)
    with pytest.raises(NativeError, match="CPU"):
        ops.distinct_hits(torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int64), 2)


@pytest.mark.parametrize("begin,end", [([0, 2, 2, 5], [2, 2, 5, 9]),            # the writer's layout, with an empty document
                                       ([0, 3, 7], [2, 5, 9]),                  # gaps between the documents
                                       ([5, 0], [9, 3])])                       # not in document order
def test_index_store_ids_are_the_repeated_document_index(begin, end):
    begin, end = np.array(begin), np.array(end)
    tokens = (torch.arange(9 * E).reshape(9, E) % 11).to(torch.float16)
    store = TokenStore(tokens, [f"d{j}" for j in range(len(begin))], begin, end)
    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device="cpu", topk_fn=_topk_fn()), distinct_fn=_distinct_fn)
    ix.index_store(store)
    rows = np.concatenate([np.arange(b, e) for b, e in zip(begin, end)])
    assert ix.inner.ids.tolist() == np.repeat(np.arange(len(begin)), end - begin).tolist()
    assert ix.inner.vectors.shape == (rows.size, 128) and ix.inner.vectors.dtype == torch.float16
    assert torch.equal(ix.inner.vectors[:, :E], tokens[rows]) and not ix.inner.vectors[:, E:].any()


# ---- two ranks under gloo ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # 10 passages, rows 0-4 on rank 0 and 5-9 on rank 1; document 77 has a passage on each shard, the better one on rank 1
    score = [4, 6, 1, 1, 1, 9, 2, 1, 1, 1]
    ids = np.array([77, 20, 21, 22, 23, 77, 24, 25, 26, 27], dtype=np.int64)
    vec = (np.array(score, dtype=np.float16)[:, None] * np.eye(E, dtype=np.float16)[0][None, :])
    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device="cpu", topk_fn=_topk_fn(), merge_fn=_merge_fn),
                     distinct_fn=_distinct_fn)
    ix.index([ids], [vec])
    assert ix.inner.vectors.shape[0] == 5
    s, i, info = ix.search(np.eye(E, dtype=np.float32)[:1], 3, index_hit_top_n=4, return_info=True)
    assert i.tolist() == [[77, 20, 24]] and s.tolist() == [[9, 6, 2]], (i, s)      # once, with its larger score
    assert info["pos"].tolist() == [[0, 1, 3]] and info["n_distinct"].tolist() == [3] and info["complete"].tolist() == [True]
    np.save(os.path.join(out_dir, f"ids{rank}.npy"), i)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_document_on_both_shards_appears_once(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (np.load(tmp_path / "ids0.npy") == np.load(tmp_path / "ids1.npy")).all()


# ---- the registered operator -------------------------------------------------------------------------------------------------
def test_fake_tensor_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from matchmaker_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        s = torch.empty(5, 100, dtype=torch.float32, device="cuda")
        i = torch.empty(5, 100, dtype=torch.int64, device="cuda")
        out = torch.ops.mm_native.distinct_hits(s, i, 7)
        assert [tuple(t.shape) for t in out] == [(5, 7), (5, 7), (5, 7), (5,), (5,)]
        assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int32, torch.int32, torch.int32]
        assert all(t.device.type == "cuda" for t in out)
