"""GPU: mm_distinct_hits_fwd through ops.distinct_hits, and retrieval.MaxPIndexer end to end.

Every comparison is bit-equality with tests/maxp_reference.py (the reference's host loop, dense_retrieval.py:414-429):
scores as int32 views, ids, positions and the two counts as they are.  The kernel selects and copies, it computes nothing,
so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from matchmaker_amd import NativeError, _lib, maxp, ops
from matchmaker_amd.retrieval import FlatIPIndexer, MaxPIndexer
from matchmaker_amd.token_store import TokenStoreWriter
from tests import maxp_reference as R
from tests import poison, util

pytestmark = pytest.mark.gpu

I64_MAX = np.iinfo(np.int64).max
NAMES = ("scores", "ids", "pos", "n_distinct", "n_valid")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_equals_reference(out, s, i, top_n, label=""):
    ref = R.distinct_hits(s, i, top_n)
    for name, got, want in zip(NAMES, out, ref):
        got = _bits(got)
        assert got.dtype == _bits(want).dtype and got.shape == want.shape, f"{label} {name}: {got.dtype} {got.shape}"
        bad = np.argwhere(got != _bits(want))
        assert bad.size == 0, f"{label} {name}: {len(bad)} elements differ from the reference, first at {bad[0].tolist()}"


def check(dev, s, i, top_n, label=""):
    s, i = np.asarray(s, dtype=np.float32), np.asarray(i, dtype=np.int64)
    assert_equals_reference(ops.distinct_hits(_dev(s, dev), _dev(i, dev), top_n), s, i, top_n, label)


def descending(rng, nq, K):
    return -np.sort(-rng.standard_normal((nq, K)).astype(np.float32), axis=1)


# ---- sizes: the powers of two, one off either side, the limit ------------------------------------------------------------
def three_rows(rng, K):
    """Row 0: about K / 3 documents with repeats and dropped slots; row 1: all distinct, ids >= 2^32; row 2: one long run of
    one id with a few others in between."""
    a = rng.integers(0, K // 3 + 1, K)
    a[rng.random(K) < 0.1] = -1
    b = (1 << 32) + rng.permutation(K).astype(np.int64) * 3
    c = np.full(K, 42, dtype=np.int64)
    c[rng.random(K) < 0.05] = 7
    c[K // 2] = 99
    return np.stack([a, b, c]).astype(np.int64)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 100, 1000, 1024, 4097, 8192])
def test_sizes(K):
    dev = util.require_gpu()
    rng = np.random.default_rng(K)
    s, i = descending(rng, 3, K), three_rows(rng, K)
    for top_n in sorted({1, max(1, round(K / 2)), K}):
        check(dev, s, i, top_n, f"K={K} top_n={top_n}")


# ---- id patterns -----------------------------------------------------------------------------------------------------------
def _patterns():
    rng = np.random.default_rng(23)
    K = 200
    p = {}
    p["all equal"] = (np.full(K, 5), 10)
    p["all distinct"] = (rng.permutation(K), 10)
    p["all -1"] = (np.full(K, -1), 10)
    a = rng.integers(0, 30, K)
    a[40:90] = -1
    a[100:110] = np.iinfo(np.int64).min
    a[110:115] = -2
    a[-20:] = -7
    p["-1 and other negatives in the middle and at the end"] = (a, 25)
    p["ids >= 2^32"] = ((1 << 32) + rng.integers(0, 40, K) * (1 << 33), 30)
    hi = rng.integers(0, 2, K).astype(np.int64) << rng.integers(32, 63, K)      # one low word, one of bits 32-62 or none
    p["ids that differ only in bits 32-62"] = (hi | 0x1234, 150)
    for n_max in (1, 2):
        b = rng.integers(0, 20, 100)
        b[::7] = -1
        b[-3:] = -1
        b[50] = I64_MAX
        if n_max == 2:
            b[10] = I64_MAX
        p[f"INT64_MAX x{n_max}, dropped slots, K = 100"] = (b, 100)
    c = rng.integers(0, 9, K)
    c[30:130] = 3                                                              # a run of 100 > 64
    p["a run longer than a wavefront"] = (c, 9)
    d = rng.integers(0, 50, 3000)
    d[700:2300] = 11                                                           # a run of 1,600 > the 1,024-thread workgroup
    p["a run longer than the workgroup"] = (d, 50)
    for extra in (-1, 0, 1):                                                   # distinct count = top_n - 1, top_n, top_n + 1
        e = rng.integers(0, 10 + extra, 100)
        e[:10 + extra] = np.arange(10 + extra)
        p[f"distinct = top_n {extra:+d}"] = (rng.permutation(e), 10)
    return p


PATTERNS = _patterns()


@pytest.mark.parametrize("name", list(PATTERNS))
def test_id_patterns(name):
    dev = util.require_gpu()
    ids, top_n = PATTERNS[name]
    ids = np.asarray(ids, dtype=np.int64)[None, :]
    if name.startswith("distinct = top_n"):
        assert len(set(ids[0].tolist())) == 10 + int(name.split()[-1])
    s = descending(np.random.default_rng(1), 1, ids.shape[1])
    for t in sorted({1, top_n, ids.shape[1]}):
        check(dev, s, ids, t, f"{name} top_n={t}")


# ---- scores are payload ------------------------------------------------------------------------------------------------------
def test_score_payloads_and_list_order():
    dev = util.require_gpu()
    rng = np.random.default_rng(4)
    K = 130
    ids = rng.integers(0, 40, (4, K)).astype(np.int64)
    s = np.empty((4, K), dtype=np.float32)
    s[0] = 1.5                                                                  # equal scores: list order decides
    s[1] = rng.standard_normal(K)                                               # an UNSORTED list: first occurrences, not maxima
    s[2] = np.sort(rng.standard_normal(K))                                      # ascending: the first occurrence is the minimum
    s[3] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0], dtype=np.float32), K)
    s[3, :6] = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0]
    ids[3, :6] = [100, 101, 102, 103, 104, 105]
    quiet = np.array([0x7fc00001, 0xffc12345], dtype=np.uint32).view(np.float32)   # NaN payload and sign bits are copied too
    s[3, 6:8], ids[3, 6:8] = quiet, [106, 107]
    for top_n in (1, 20, K):
        check(dev, s, ids, top_n, f"payload top_n={top_n}")
    out = ops.distinct_hits(_dev(s, dev), _dev(ids, dev), K)
    got = out[0][3, :8].cpu().numpy().view(np.uint32)
    assert got.tolist() == s[3, :8].view(np.uint32).tolist()


# ---- the grid ----------------------------------------------------------------------------------------------------------------
def test_no_query():
    dev = util.require_gpu()
    out = ops.distinct_hits(torch.empty(0, 50, device=dev), torch.empty(0, 50, dtype=torch.int64, device=dev), 5)
    assert [tuple(t.shape) for t in out] == [(0, 5), (0, 5), (0, 5), (0,), (0,)]
    s, i = torch.zeros(1, 8, device=dev), torch.zeros(1, 8, dtype=torch.int64, device=dev)
    rc = _lib.lib().mm_distinct_hits_fwd(s.data_ptr(), i.data_ptr(), 0, 8, 2, None, None, None, None, None,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.MM_OK                                                     # nq = 0: no launch, the pointers are not looked at


def test_more_queries_than_a_grid_y_holds():
    dev = util.require_gpu()
    rng = np.random.default_rng(70)
    nq = 70000                                                                  # > 65,535
    ids = rng.integers(-1, 2, (nq, 2)).astype(np.int64)
    s = descending(rng, nq, 2)
    check(dev, s, ids, 2, "nq=70000")
    check(dev, s, ids, 1, "nq=70000 top_n=1")


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,top_n", [(0, 1), (8193, 1), (8, 0), (8, 9)])
def test_refusals_leave_the_outputs_untouched(K, top_n):
    dev = util.require_gpu()
    L = _lib.lib()
    # the entry point itself: refused before any launch, so the 8-column buffers are never addressed with the claimed K
    s, i = torch.zeros(2, 8, device=dev), torch.zeros(2, 8, dtype=torch.int64, device=dev)
    outs = [torch.full((2 * 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev) for _ in range(5)]
    rc = L.mm_distinct_hits_fwd(s.data_ptr(), i.data_ptr(), 2, K, top_n, *[o.data_ptr() for o in outs],
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.MM_EUNSUPPORTED, L.mm_last_error()
    assert all(bool((o == 0x5A5A5A5A).all()) for o in outs)
    # the wrapper restates the limits
    with pytest.raises(NativeError) as e:
        ops.distinct_hits(torch.zeros(2, K, device=dev), torch.zeros(2, K, dtype=torch.int64, device=dev), top_n)
    assert e.value.code == _lib.MM_EUNSUPPORTED


def test_invalid_arguments():
    dev = util.require_gpu()
    L = _lib.lib()
    s, i = torch.zeros(1, 8, device=dev), torch.zeros(1, 8, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert L.mm_distinct_hits_fwd(s.data_ptr(), i.data_ptr(), -1, 8, 2, None, None, None, None, None, st) == _lib.MM_EINVAL
    assert L.mm_distinct_hits_fwd(s.data_ptr(), i.data_ptr(), 1, 8, 2, None, None, None, None, None, st) == _lib.MM_EINVAL
    for bad in [(s.double(), i, 2), (s, i.int(), 2), (s, i[:, :4], 2), (s[0], i[0], 2)]:
        with pytest.raises(NativeError):
            ops.distinct_hits(*bad)


# ---- the wrapper and the registered operator ---------------------------------------------------------------------------------
def test_non_contiguous_inputs_and_the_registered_operator():
    dev = util.require_gpu()
    from matchmaker_amd import torch_ops  # noqa: F401
    rng = np.random.default_rng(9)
    big_s, big_i = descending(rng, 4, 300), rng.integers(-1, 60, (4, 300)).astype(np.int64)
    ds, di = _dev(big_s, dev)[:, ::3], _dev(big_i, dev).t().contiguous().t()[:, ::3]
    assert not ds.is_contiguous() and not di.is_contiguous()
    assert_equals_reference(ops.distinct_hits(ds, di, 17), big_s[:, ::3], big_i[:, ::3], 17, "strided")
    assert_equals_reference(torch.ops.mm_native.distinct_hits(ds, di, 17), big_s[:, ::3], big_i[:, ::3], 17, "torch.ops")


def test_two_calls_and_a_captured_replay_give_the_same_bits():
    dev = util.require_gpu()
    rng = np.random.default_rng(31)
    K, top_n = 1000, 100
    s0, i0 = descending(rng, 5, K), rng.integers(-1, 400, (5, K)).astype(np.int64)
    s1, i1 = descending(rng, 5, K), rng.integers(-1, 90, (5, K)).astype(np.int64)      # some rows end in the fill
    s, i = _dev(s0, dev), _dev(i0, dev)

    def fn():
        return ops.distinct_hits(s, i, top_n)
    first, second = fn(), fn()
    poison.assert_same_bits(first, second, "two calls")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # warm-up off the default stream, as torch.cuda.graph asks
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # one launch: no parallel branches
        out = fn()
    s.copy_(_dev(s1, dev))             # the inputs are overwritten in place, the outputs wiped
    i.copy_(_dev(i1, dev))
    for t in out:
        t.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    assert_equals_reference(out, s1, i1, top_n, "captured replay")


# ---- poisoned memory ---------------------------------------------------------------------------------------------------------
def test_every_output_is_written_whatever_the_memory_held():
    dev = util.require_gpu()
    rng = np.random.default_rng(12)
    K, top_n = 100, 7
    s0, i0 = descending(rng, 4, K), rng.integers(-1, 30, (4, K)).astype(np.int64)
    i0[1] = -1                                                                  # a row with no valid hit: all fill
    i0[2] = 8                                                                   # one document: six fill slots
    s, i = _dev(s0, dev), _dev(i0, dev)
    outs = []
    for p in poison.POISONS:
        out, arena = poison.run(lambda: maxp.distinct_hits(s, i, top_n), p, module=maxp, label=f"distinct_hits [{p:#04x}]")
        assert len(arena.allocations) == 5, "the five outputs came from the arena; there is no workspace"
        outs.append(out)
    poison.assert_same_bits(outs[0], outs[1], "distinct_hits")
    assert_equals_reference(outs[0], s0, i0, top_n, "under poison")
    assert np.array_equal(_bits(s), _bits(s0)) and np.array_equal(_bits(i), i0), "the inputs are unchanged"


# ---- end to end --------------------------------------------------------------------------------------------------------------
E, TOP_N, HITS = 128, 10, 16


def _collection():
    """40 documents of 1-30 passages, small-integer fp16 vectors (every dot product is an integer below 2^24: exact in fp32
    in any order).  Document 0's 30 passages are query 0 with one coordinate zeroed: they fill query 0's first 16 hits.
    Documents 5 and 9 both hold a copy of query 1 (a tie at the top of its ranking, between documents), and documents 12
    and 30 share another passage."""
    rng = np.random.default_rng(40)
    n_pass = rng.integers(1, 31, 40)
    n_pass[0] = 30
    queries = rng.integers(-2, 3, (3, E)).astype(np.float32)
    docs = []
    for d, n in enumerate(n_pass):
        v = rng.integers(-2, 3, (n, E)).astype(np.float32)
        v[np.abs(v).sum(axis=1) == 0, 0] = 1                                    # no all-zero passage: the store drops those
        docs.append(v)
    nz = np.nonzero(queries[0])[0]
    for j in range(30):
        docs[0][j] = queries[0]
        docs[0][j, nz[j]] = 0
    docs[5][0] = docs[9][0] = queries[1]
    docs[30][0] = docs[12][0]
    return queries, docs


def _assert_rows(got_s, got_i, ref, rows=None, label=""):
    rs, ri = ref[0], ref[1]
    gs, gi = got_s.cpu().numpy(), got_i.cpu().numpy()
    if rows is None:
        assert np.array_equal(gi, ri), f"{label}: ids"
        assert np.array_equal(gs.view(np.int32), rs.view(np.int32)), f"{label}: scores"
        return
    for q, n in enumerate(rows):                                                # the kept prefix of every query
        assert np.array_equal(gi[q, :n], ri[q, :n]) and np.array_equal(gs[q, :n].view(np.int32), rs[q, :n].view(np.int32)), \
            f"{label}: query {q}, first {n} documents"
        assert (gi[q, n:] == -1).all() and np.isneginf(gs[q, n:]).all(), f"{label}: query {q}, the fill"


@pytest.mark.parametrize("route", ["index_resident", "index_store"])
def test_documents_from_passage_hits_end_to_end(route):
    dev = util.require_gpu()
    queries, docs = _collection()
    vectors = np.concatenate(docs)
    doc_of = np.repeat(np.arange(len(docs)), [len(d) for d in docs]).astype(np.int64)
    # the reference first: what one search of 16 hits must show, and the exact answer
    hs, hi, _ = R.topk_hits(queries, vectors, doc_of, HITS)
    ref16 = R.distinct_hits(hs, hi, TOP_N)
    assert ref16[3][0] == 1 and (ref16[3] < TOP_N).any(), "query 0's 16 hits are all document 0's"
    brute = R.brute_force(queries, vectors, doc_of, TOP_N)
    assert (brute[3] >= TOP_N).all() and set(brute[1][1, :2].tolist()) == {5, 9} and brute[0][1, 0] == brute[0][1, 1]

    ix = MaxPIndexer(FlatIPIndexer({"token_dim": E}, device=dev), max_hits=4096)
    if route == "index_resident":
        ix.index_resident(_dev(doc_of, dev), _dev(vectors, dev).to(torch.float16))
    else:
        w = TokenStoreWriter(len(docs) * 30, E, dtype=torch.float16, device=dev)
        for a in range(0, len(docs), 16):                                       # [docs, chunks, dim] batches, zero rows = padding
            batch = np.zeros((len(docs[a:a + 16]), 30, E), dtype=np.float32)
            for j, d in enumerate(docs[a:a + 16]):
                batch[j, 30 - len(d):] = d                                      # the padding in front: "wherever they are"
            w.append(list(range(a, a + batch.shape[0])), _dev(batch, dev).to(torch.float16))
        ix.index_store(w.finish())
        assert torch.equal(ix.inner.ids.cpu(), torch.from_numpy(doc_of))
    q = _dev(queries, dev)

    s, i, info = ix.search_device(q, TOP_N, index_hit_top_n=HITS, return_info=True)
    complete = info["complete"].cpu().numpy()
    assert np.array_equal(info["n_distinct"].cpu().numpy(), ref16[3])
    assert np.array_equal(complete, ref16[3] >= TOP_N) and not complete.all()
    _assert_rows(s, i, brute, rows=np.minimum(ref16[3], TOP_N), label="16 hits")
    assert np.array_equal(info["pos"].cpu().numpy(), ref16[2])

    s, i, info = ix.search_device(q, TOP_N, index_hit_top_n=HITS, widen=True, return_info=True)
    assert bool(info["complete"].all())
    assert (info["hits_used"].cpu().numpy()[complete] == HITS).all() and (info["hits_used"].cpu().numpy()[~complete] > HITS).all()
    _assert_rows(s, i, brute, label="widened")
    hs_np, hi_np = ix.search(queries, TOP_N, index_hit_top_n=HITS, widen=True)
    assert np.array_equal(hi_np, brute[1]) and np.array_equal(hs_np.view(np.int32), brute[0].view(np.int32))
