"""GPU test of the one thing ops._call could get wrong: the stream and the workspace an operator's native call gets.  Every
scoring and retrieval operator that goes through the helper is called on a side stream, at a tiny shape whose workspace is not empty and at
one whose workspace query exceeds the 65,536-byte floor of the cached buffers, and must return the bits of the same calls on
the default stream.  Operators whose policy is a fresh workspace must leave the cache ops._WS alone; the cached ones must
replace their first buffer when the second call needs a larger one.  The forwards whose entry points need no workspace
(PACRR, CO-PACRR, DRMM) are held to the same bits and to leaving the cache alone; MatchPyramid's workspace is empty at the tiny
shape by construction (a slot exists only for an activation plane that does not fit the LDS, so the smallest non-empty
workspace is larger than the floor): it is called at the tiny shape without one and at a shape with one.  The flat top-k
operators allocate fresh and exceed the floor already at the tiny shape (two candidate lists of 4,096 entries per query); the
retrieval operators whose entry points end in the stream alone are held like the other forwards without a workspace."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

FLOOR = 1 << 16
TINY = 3               # pairs of the tiny shape: B = 3, Q = 5, D = 7, E = 128 (kernel pooling: E = 100)
Q, D = 5, 7


def _mask(rows, L, gen, dev):
    """dense uint8 prefix masks with at least one real token per row"""
    n = torch.randint(1, L + 1, (rows,), generator=gen)
    return (torch.arange(L)[None] < n[:, None]).to(torch.uint8).to(dev)


def _emb(gen, dev, dtype, *shape):
    return torch.randn(*shape, generator=gen).to(dtype).to(dev)


def _rbf(dev, rows=1):
    mu = torch.tensor([1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9], device=dev)
    return mu, torch.full((11,), 0.1, device=dev), torch.linspace(0.5, 1.5, 11, device=dev), \
        torch.linspace(-1.0, 1.0, 11 * rows, device=dev).reshape(rows, 11)


# ---- operator -> (workspace bytes of the call, the call); B = the shape's pair count ----------------------------------------
def _maxsim(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.bfloat16, B, Q, 128), _emb(gen, dev, torch.bfloat16, B, D, 128)
    qm, dm = _mask(B, Q, gen, dev), _mask(B, D, gen, dev)
    return L.mm_maxsim_workspace_bytes(B, 1, Q, D, K, K), lambda: (ops.maxsim(q, d, qm, dm),)


def _maxsim_bwd(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.float16, B, Q, 128), _emb(gen, dev, torch.float16, B, D, 128)
    qm, dm, go = _mask(B, Q, gen, dev), _mask(B, D, gen, dev), _emb(gen, dev, torch.float32, B)
    return L.mm_maxsim_bwd_workspace_bytes(B, Q, D, K, K), lambda: ops.maxsim_bwd(q, d, qm, dm, go)


def _maxsim_inbatch(ops, L, K, dev, gen, B):
    Bq, Bd = (B, B) if B == TINY else (64, B)
    q, d = _emb(gen, dev, torch.bfloat16, Bq, Q, 128), _emb(gen, dev, torch.bfloat16, Bd, D, 128)
    qm, dm = _mask(Bq, Q, gen, dev), _mask(Bd, D, gen, dev)
    return L.mm_maxsim_inbatch_workspace_bytes(Bq, Bd, Q, D, K, K), lambda: (ops.maxsim_inbatch(q, qm, d, dm),)


def _maxsim_inbatch_bwd(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.bfloat16, B, Q, 128), _emb(gen, dev, torch.bfloat16, B, D, 128)
    qm, dm, go = _mask(B, Q, gen, dev), _mask(B, D, gen, dev), _emb(gen, dev, torch.float32, B, B)
    return L.mm_maxsim_inbatch_bwd_workspace_bytes(B, B, Q, D, 128, K, K), lambda: ops.maxsim_inbatch_bwd(q, qm, d, dm, go)


def _ragged_inputs(dev, gen, B):
    q, qm = _emb(gen, dev, torch.float16, B, Q, 128), _mask(B, Q, gen, dev)
    n = torch.randint(1, D + 1, (B,), generator=gen)
    end = torch.cumsum(n, 0)
    return q, qm, _emb(gen, dev, torch.float16, int(end[-1]), 128), (end - n).to(dev), end.to(dev)


def _maxsim_ragged(ops, L, K, dev, gen, B):
    q, qm, tokens, begin, end = _ragged_inputs(dev, gen, B)
    return L.mm_maxsim_ragged_workspace_bytes(B, 1, Q, K), lambda: (ops.maxsim_ragged(q, tokens, begin, end, qm, check_ranges=False),)


def _maxsim_ragged_fp8(ops, L, K, dev, gen, B):
    q, qm, tokens, begin, end = _ragged_inputs(dev, gen, B)
    codes, scales = ops.fp8_quantize_rows(tokens)
    return L.mm_maxsim_ragged_fp8_workspace_bytes(B, 1, Q, K), \
        lambda: (ops.maxsim_ragged_fp8(q, codes, scales, begin, end, qm, check_ranges=False),)


def _kernel_pool(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.float32, B, Q, 100), _emb(gen, dev, torch.float32, B, D, 100)
    qm, dm = _mask(B, Q, gen, dev), _mask(B, D, gen, dev)
    mu, sigma, alpha, w = _rbf(dev)
    return L.mm_kernel_pool_workspace_bytes(B, 1, Q, D, K, K), lambda: (ops.kernel_pool(q, d, qm, dm, mu, sigma, alpha, w),)


def _kernel_pool_multi(ops, L, K, dev, gen, B):
    qs = [_emb(gen, dev, torch.float32, B, Q, 100) for _ in range(2)]
    ds = [_emb(gen, dev, torch.float32, B, D, 100) for _ in range(2)]
    qm, dm = _mask(B, Q, gen, dev), _mask(B, D, gen, dev)
    mu, sigma, alpha, w = _rbf(dev, rows=4)
    return L.mm_kernel_pool_multi_workspace_bytes(B, 1, 2, 2, Q, D, K, K), \
        lambda: (ops.kernel_pool_multi(qs, ds, qm, dm, mu, sigma, alpha, w),)


def _kernel_pool_bwd(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.float32, B, Q, 100), _emb(gen, dev, torch.float32, B, D, 100)
    qm, dm, go = _mask(B, Q, gen, dev), _mask(B, D, gen, dev), _emb(gen, dev, torch.float32, B)
    mu, sigma, alpha, w = _rbf(dev)
    return L.mm_kernel_pool_bwd_workspace_bytes2(B, Q, D, 100, K, K), lambda: ops.kernel_pool_bwd(q, d, qm, dm, mu, sigma, alpha, w, go)


def _tkl_inputs(dev, B):
    from tests.test_tkl_gpu import _epilogue_inputs       # float masks: TKL takes no other kind
    return _epilogue_inputs(dev, B, Q, D, 128, "embedding", 31)


def _tkl_score(ops, L, K, dev, gen, B):
    q_ctx, chunks, cmask, slot, qm, params, B, C, sat = _tkl_inputs(dev, B)
    return L.mm_tkl_workspace_bytes(B, chunks.shape[0], C, Q, 11), \
        lambda: ops.tkl_score(q_ctx, chunks, cmask, slot, qm, params, B, C, 11, sat, return_windows=True, check_order=False)


def _tkl_bwd(ops, L, K, dev, gen, B):
    q_ctx, chunks, cmask, slot, qm, params, B, C, sat = _tkl_inputs(dev, B)
    _, win = ops.tkl_score(q_ctx, chunks, cmask, slot, qm, params, B, C, 11, sat, return_windows=True, check_order=False)
    go = _emb(gen, dev, torch.float32, B)
    return L.mm_tkl_bwd_workspace_bytes2(B, C, Q, 128), lambda: ops.tkl_bwd(q_ctx, chunks, cmask, slot, qm, params, win, go, B, C, 11, sat)


def _pacrr_inputs(dev, gen, B):
    return (_emb(gen, dev, torch.float32, B, Q, 128), _emb(gen, dev, torch.float32, B, D, 128),
            [_emb(gen, dev, torch.float32, 4, 1, 2, 2)], [_emb(gen, dev, torch.float32, 4)])


def _pacrr_kmax_bwd(ops, L, K, dev, gen, B):
    q, d, w, b = _pacrr_inputs(dev, gen, B)
    _, idx = ops.pacrr_kmax(q, d, w, b, 2, save=True)
    go = _emb(gen, dev, torch.float32, B, Q, 4)

    def run():
        gq, gd, gw, gb = ops.pacrr_kmax_bwd(q, d, w, idx, go, 2)
        return gq, gd, *gw, *gb
    return L.mm_pacrr_workspace_bytes(B, Q, D, 4, 2, 2), run


def _co_pacrr_kmax_bwd(ops, L, K, dev, gen, B):
    q, d, w, b = _pacrr_inputs(dev, gen, B)
    views = [2, 4, 6, 7]
    _, idx = ops.co_pacrr_kmax(q, d, w, b, 2, views, save=True)
    go = _emb(gen, dev, torch.float32, B, Q, 32)

    def run():
        gq, gd, gw, gb = ops.co_pacrr_kmax_bwd(q, d, w, idx, go, 2, views)
        return gq, gd, *gw, *gb
    return L.mm_co_pacrr_workspace_bytes(B, Q, D, 128, 4, 2, 2), run


def _pacrr_kmax(ops, L, K, dev, gen, B):
    q, d, w, b = _pacrr_inputs(dev, gen, B)
    return 0, lambda: ops.pacrr_kmax(q, d, w, b, 2, save=True)


def _co_pacrr_kmax(ops, L, K, dev, gen, B):
    q, d, w, b = _pacrr_inputs(dev, gen, B)
    return 0, lambda: ops.co_pacrr_kmax(q, d, w, b, 2, [2, 4, 6, 7], save=True)


def _drmm_score(ops, L, K, dev, gen, B):
    q, d = _emb(gen, dev, torch.float32, B, Q, 128), _emb(gen, dev, torch.float32, B, D, 128)
    gate = torch.softmax(_emb(gen, dev, torch.float32, B, Q), -1)
    W1, b1, w2, b2 = (_emb(gen, dev, torch.float32, *sh) for sh in ((10, 10), (10,), (10,), (1,)))
    return L.mm_drmm_workspace_bytes(B, Q, D, 128, 10), lambda: ops.drmm_score(q, d, gate, W1, b1, w2, b2, return_hist=True)


def _matchpyramid_features(ops, L, K, dev, gen, B):
    Qm, Dm, E, C = (Q, D, 128, 4) if B == TINY else (64, 700, 64, 16)      # 16 planes of 64 x 700 floats do not fit the LDS
    q, d = _emb(gen, dev, torch.float32, B, Qm, E), _emb(gen, dev, torch.float32, B, Dm, E)
    w, b, pools = [_emb(gen, dev, torch.float32, C, 1, 3, 3)], [_emb(gen, dev, torch.float32, C)], [(2, 2)]
    layers, _ = ops._mp_layers(Qm, Dm, w, b, pools, "matchpyramid_features")
    return ops.mm_matchpyramid_workspace_bytes(B, Qm, Dm, 1, *layers), lambda: (ops.matchpyramid_features(q, d, w, b, pools),)


# ---- retrieval: the tiny shape is 3 queries against 40 store rows in 4 lists, nprobe 2, E = 128, fp16, k = 2; the second one
# 64 queries against 2,000 rows (the flat top-k: 5,000, past the 4,096 rows up to which every row is a candidate)
RK = 2


def _store(dev, gen, B, n_big=2000):
    """(queries [nq, 128], rows [n, 128], list_begin [5], probes [nq, 2] of distinct lists)"""
    nq, n = (3, 40) if B == TINY else (64, n_big)
    lb = torch.arange(5, dtype=torch.int64) * (n // 4)
    probes = torch.stack([torch.randperm(4, generator=gen)[:2] for _ in range(nq)]).to(torch.int32)
    return _emb(gen, dev, torch.float16, nq, 128), _emb(gen, dev, torch.float16, n, 128), lb.to(dev), probes.to(dev)


def _dot_topk(ops, L, K, dev, gen, B):
    q, x, _, _ = _store(dev, gen, B, 5000)
    return L.mm_dot_topk_workspace_bytes(x.shape[0], q.shape[0], RK), lambda: ops.dot_topk(q, x, RK)


def _dot_topk_fp8(ops, L, K, dev, gen, B):
    q, x, _, _ = _store(dev, gen, B, 5000)
    codes, scales = ops.fp8_quantize_rows(x)
    return L.mm_dot_topk_fp8_workspace_bytes(x.shape[0], q.shape[0], RK), lambda: ops.dot_topk_fp8(q, codes, scales, RK)


def _ivf_scan(ops, L, K, dev, gen, B):
    q, x, lb, probes = _store(dev, gen, B)
    return L.mm_ivf_scan_workspace_bytes(x.shape[0], 4, q.shape[0], 2, RK), lambda: ops.ivf_scan(q, x, lb, probes, RK)


def _ivf_scan_fp8(ops, L, K, dev, gen, B):
    q, x, lb, probes = _store(dev, gen, B)
    codes, scales = ops.fp8_quantize_rows(x)
    return L.mm_ivf_scan_fp8_workspace_bytes(x.shape[0], 4, q.shape[0], 2, RK), \
        lambda: ops.ivf_scan_fp8(q, codes, scales, lb, probes, RK)


def _codebook(dev, gen):
    return _emb(gen, dev, torch.float16, 64, 16, 2)


def _ah_scan(ops, L, K, dev, gen, B):
    q, x, lb, probes = _store(dev, gen, B)
    codes = torch.randint(0, 256, (x.shape[0], 32), generator=gen).to(torch.uint8).to(dev)
    book, ps = _codebook(dev, gen), _emb(gen, dev, torch.float32, q.shape[0], 2)
    return L.mm_ah_scan_workspace_bytes(x.shape[0], 4, q.shape[0], 2, RK), lambda: ops.ah_scan(q, codes, book, lb, probes, ps, RK)


def _graph_search(ops, L, K, dev, gen, B):
    # tiny: the visited table fits the LDS (a 256-byte workspace); second shape: one slice of global memory per query
    nq, n, M, ef, width, n_entry, iters = (3, 40, 4, 8, 2, 2, 12) if B == TINY else (64, 20000, 32, 64, 4, 8, 64)
    q, x = _emb(gen, dev, torch.float16, nq, 128), _emb(gen, dev, torch.float16, n, 128)
    nbr = torch.randint(0, n, (n, M), generator=gen).to(torch.int32).to(dev)
    entry = torch.randint(0, n, (nq, n_entry), generator=gen).to(torch.int32).to(dev)
    return L.mm_graph_search_workspace_bytes(n, nq, M, ef, width, n_entry, iters), \
        lambda: ops.graph_search(q, x, nbr, entry, ef, RK, width=width, max_iters=iters, return_stats=True)


def _kmeans_segment_sum(ops, L, K, dev, gen, B):
    n = 40 if B == TINY else 70000                             # 3 lists: 136 chunks of 512 rows at the second shape
    x = _emb(gen, dev, torch.float16, n, 128)
    order = torch.randperm(n, generator=gen).to(dev)
    lb = torch.tensor([0, n // 3, 2 * n // 3, n], dtype=torch.int64, device=dev)
    return L.mm_kmeans_segment_sum_workspace_bytes(n, 3, 128), lambda: (ops.kmeans_segment_sum(x, order, lb),)


def _colbert_candidates(ops, L, K, dev, gen, B):
    nq, H, n_docs, T = (3, 8, 5, 40) if B == TINY else (64, 512, 50, 2000)
    hits = torch.randint(-1, T, (nq, H), generator=gen).to(dev)
    begin = (torch.arange(n_docs, dtype=torch.int64) * (T // n_docs)).to(dev)
    doc_of = torch.randperm(n_docs, generator=gen).to(torch.int32).to(dev)
    return L.mm_colbert_candidates_workspace_bytes(nq, H), lambda: ops.colbert_candidates(hits, begin, begin + T // n_docs, doc_of, T)


def _ah_encode(ops, L, K, dev, gen, B):
    _, x, _, _ = _store(dev, gen, B)
    lists = torch.randint(0, 4, (x.shape[0],), generator=gen).to(torch.int32).to(dev)
    cent, book = _emb(gen, dev, torch.float16, 4, 128), _codebook(dev, gen)
    return 0, lambda: (ops.ah_encode(x, lists, cent, book, 4.0),)


def _gather_dot(ops, L, K, dev, gen, B):
    q, x, _, _ = _store(dev, gen, B)
    rows = torch.randint(-1, x.shape[0], (q.shape[0], 70), generator=gen).to(dev)      # two workgroups per query
    return 0, lambda: (ops.gather_dot(q, x, rows),)


def _kmeans_assign(ops, L, K, dev, gen, B):
    _, x, _, _ = _store(dev, gen, B)
    cent = _emb(gen, dev, torch.float16, 4, 128)
    return 0, lambda: ops.kmeans_assign(x, cent)


def _topk_merge(ops, L, K, dev, gen, B):
    nq = 3 if B == TINY else 64
    scores = _emb(gen, dev, torch.float32, nq, 6)
    ids = torch.randint(-1, 1000, (nq, 6), generator=gen).to(dev)
    return 0, lambda: ops.topk_merge(scores, ids, RK)


def _fp8_quantize_rows(ops, L, K, dev, gen, B):
    _, x, _, _ = _store(dev, gen, B)
    return 0, lambda: ops.fp8_quantize_rows(x)


CACHED, FRESH, FRESH_TINY_EMPTY, NO_WORKSPACE = "cached", "fresh", "fresh, empty at the tiny shape", "no workspace"
FRESH_TINY_ABOVE_FLOOR = "fresh, above the floor already at the tiny shape"

# operator -> (builder, pairs of the second shape (its workspace exceeds the floor where the operator has one), workspace policy)
CASES = {
    "maxsim": (_maxsim, 4200, CACHED),
    "maxsim_bwd": (_maxsim_bwd, 4200, CACHED),
    "maxsim_inbatch_bwd": (_maxsim_inbatch_bwd, 100, CACHED),
    "kernel_pool": (_kernel_pool, 4200, CACHED),
    "maxsim_inbatch": (_maxsim_inbatch, 8300, FRESH),        # 64 queries x 8300 documents
    "maxsim_ragged": (_maxsim_ragged, 8300, FRESH),
    "maxsim_ragged_fp8": (_maxsim_ragged_fp8, 8300, FRESH),
    "kernel_pool_multi": (_kernel_pool_multi, 2200, FRESH),
    "kernel_pool_bwd": (_kernel_pool_bwd, 300, FRESH),
    "tkl_score": (_tkl_score, 40, FRESH),
    "tkl_bwd": (_tkl_bwd, 40, FRESH),
    "pacrr_kmax_bwd": (_pacrr_kmax_bwd, 600, FRESH),
    "co_pacrr_kmax_bwd": (_co_pacrr_kmax_bwd, 600, FRESH),
    "matchpyramid_features": (_matchpyramid_features, 2, FRESH_TINY_EMPTY),
    "pacrr_kmax": (_pacrr_kmax, 600, NO_WORKSPACE),
    "co_pacrr_kmax": (_co_pacrr_kmax, 600, NO_WORKSPACE),
    "drmm_score": (_drmm_score, 600, NO_WORKSPACE),
    # retrieval (the second number only says "not the tiny shape": the builders above choose the shapes)
    "ivf_scan": (_ivf_scan, 64, CACHED),
    "ivf_scan_fp8": (_ivf_scan_fp8, 64, CACHED),
    "ah_scan": (_ah_scan, 64, CACHED),
    "graph_search": (_graph_search, 64, CACHED),
    "kmeans_segment_sum": (_kmeans_segment_sum, 70000, CACHED),
    "colbert_candidates": (_colbert_candidates, 64, CACHED),
    "dot_topk": (_dot_topk, 64, FRESH_TINY_ABOVE_FLOOR),
    "dot_topk_fp8": (_dot_topk_fp8, 64, FRESH_TINY_ABOVE_FLOOR),
    "ah_encode": (_ah_encode, 64, NO_WORKSPACE),
    "gather_dot": (_gather_dot, 64, NO_WORKSPACE),
    "kmeans_assign": (_kmeans_assign, 64, NO_WORKSPACE),
    "topk_merge": (_topk_merge, 64, NO_WORKSPACE),
    "fp8_quantize_rows": (_fp8_quantize_rows, 64, NO_WORKSPACE),
}


@pytest.mark.parametrize("op", list(CASES))
def test_side_stream_calls_equal_the_default_stream_and_keep_the_workspace_policy(op):
    from matchmaker_amd import ops, _lib
    dev = util.require_gpu()
    build, big, policy = CASES[op]
    L = _lib.lib()
    gen = torch.Generator().manual_seed(17)
    ops.clear_workspaces()
    calls = [build(ops, L, _lib.MASK_U8, dev, gen, B) for B in (TINY, big)]
    (wsb_tiny, _), (wsb_big, _) = calls
    print(f"{op}: workspace {wsb_tiny} bytes at {TINY} pairs, {wsb_big} bytes at {big}")
    if policy == NO_WORKSPACE:
        assert wsb_tiny == 0 and wsb_big == 0
    elif policy == FRESH_TINY_EMPTY:
        assert wsb_tiny == 0 and FLOOR < wsb_big
    elif policy == FRESH_TINY_ABOVE_FLOOR:
        assert FLOOR < wsb_tiny <= wsb_big
    else:
        assert 0 < wsb_tiny <= FLOOR < wsb_big
    want = [run() for _, run in calls]                         # default stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    key = (dev.index, side.cuda_stream)
    before = set(ops._WS)
    assert key not in before
    side.wait_stream(torch.cuda.current_stream())
    got, bufs = [], []
    with torch.cuda.stream(side):
        for _, run in calls:
            got.append(run())
            bufs.append(ops._WS.get(key))
    side.synchronize()
    for w, g in zip(want, got):
        assert len(w) == len(g)
        for a, b in zip(w, g):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if policy == CACHED:
        assert bufs[0] is not None and bufs[0].numel() == FLOOR
        assert bufs[1] is not bufs[0] and bufs[1].numel() >= wsb_big and ops._WS[key] is bufs[1]
    else:
        assert set(ops._WS) == before and bufs == [None, None]
