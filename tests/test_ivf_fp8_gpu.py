"""GPU tests of the fp8 IVF list scan (ops.ivf_scan_fp8 = mm_ivf_scan_fp8_fwd), of IVFFp8IPIndexer and of
TokenStore.build_token_index on an fp8-only store, against the float64 restatement of tests/ivf_fp8_reference.py.  On the
exact (scaled) store every score is exact in fp32 in any summation order (tests/test_ivf_fp8_cpu.py), so scores AND rows are
compared bit for bit, tie order and padding included; on random data every score is held to
(E + 2) 2^-24 scales[t] sum_k |q_k| |deq_tk| of float64."""
import functools

import numpy as np
import pytest
import torch

from tests import fp8_store_reference as F
from tests import fp8_token_search_reference as R
from tests import ivf_fp8_reference as I8
from tests import ivf_reference as IR
from tests import util

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _dev(*arrays):
    dev = util.require_gpu()
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@functools.lru_cache(maxsize=None)
def _exact(E, nq, k):
    """inputs and restatement of one exact case, computed once for both query dtypes and never modified"""
    q, codes, scales, lb, probes = I8.exact_problem(E, nq, I8.EXACT_NPROBE, I8.exact_seed(E, nq, k))
    ref_s, ref_r = I8.ivf_scan_fp8(q, codes, scales, lb, probes, k, full=R.scores64(q, codes, scales))
    return q, codes, scales, lb, probes, ref_s.astype(np.float32), ref_r


def _scan(q, codes, scales, lb, probes, k, dtype):
    from matchmaker_amd import ops
    qd, cd, sd, lbd, pd = _dev(q, codes, scales, lb, probes)
    s, r = ops.ivf_scan_fp8(qd.to(dtype), cd, sd, lbd, pd, k)
    return s.cpu().numpy(), r.cpu().numpy()


# ---- 1. the exact store, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,nq,k", I8.EXACT)
def test_scan_equals_the_restatement_bit_for_bit_on_the_exact_store(dtype, E, nq, k):
    q, codes, scales, lb, probes, ref_s, ref_r = _exact(E, nq, k)
    s, r = _scan(q, codes, scales, lb, probes, k, dtype)
    assert s.dtype == np.float32 and r.dtype == np.int64 and s.shape == (nq, k)
    assert np.array_equal(r, ref_r), f"rows differ in {int((r != ref_r).sum())} places"
    assert np.array_equal(s, ref_s)                                        # (-inf pads compare equal)


def test_more_ties_at_the_kth_score_than_fit_keep_the_lowest_rows():
    """tests/ivf_reference.py's tie problem, quantised: identical rows have identical codes and scales, so the 40 rows still
    tie from rank 8 on and the three lowest of them close the ten results."""
    q, codes, scales, lb, probes, k, group = I8.tie_problem()
    s, r = _scan(q, codes, scales, lb, probes, k, torch.float16)
    ref_s, ref_r = I8.ivf_scan_fp8(q, codes, scales, lb, probes, k)
    assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32))
    assert r[0, 7:].tolist() == group[:3].tolist() and (s[0, 7:] == s[0, 7]).all() and s[0, 6] > s[0, 7]


# ---- 2. the same bits as the 16-bit scan over the dequantised rows ----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,nq,k", [(128, 37, 10), (768, 37, 1000)])
def test_scan_equals_the_16_bit_scan_of_the_dequantised_rows(dtype, E, nq, k):
    from matchmaker_amd import ops
    q, codes, scales, lb, probes, _, _ = _exact(E, nq, k)
    qd, cd, sd, lbd, pd = _dev(q, codes, scales, lb, probes)
    s8, r8 = ops.ivf_scan_fp8(qd.to(dtype), cd, sd, lbd, pd, k)
    v = ops.fp8_dequantize_rows(cd, sd, torch.float16).to(dtype)           # (|value| <= 64: exact in both types)
    s16, r16 = ops.ivf_scan(qd.to(dtype), v, lbd, pd, k)
    assert torch.equal(s8, s16) and torch.equal(r8, r16)


# ---- 3. unions shorter than k ----------------------------------------------------------------------------------------------
def test_scan_pads_short_unions_and_unprobed_queries():
    q, codes, scales = R.scaled_store(5, I8.N_ROWS, 256, 11)
    lb, probes, k = I8.list_begin(), I8.short_union_probes(), 100
    s, r = _scan(q, codes, scales, lb, probes, k, torch.float16)
    ref_s, ref_r = I8.ivf_scan_fp8(q, codes, scales, lb, probes, k)
    assert [(x >= 0).sum() for x in r] == I8.SHORT_FOUND
    assert np.array_equal(r, ref_r) and np.array_equal(s, ref_s.astype(np.float32))
    assert all((x[n:] == -1).all() and np.isneginf(y[n:]).all() for x, y, n in zip(r, s, I8.SHORT_FOUND))


# ---- 4. interior views, guard bytes, the workspace refusal -------------------------------------------------------------------
def test_interior_views_guards_and_a_short_workspace():
    from matchmaker_amd import _lib, ops
    dev = util.require_gpu()
    E, nq, k = 128, 37, 10
    q, codes, scales, lb, probes, ref_s, ref_r = _exact(E, nq, k)
    n = codes.shape[0]
    qd, cd, sd, lbd, pd = _dev(q, codes, scales, lb, probes)
    qd = qd.half()
    # the store as a view into larger buffers whose surrounding rows are NaN codes (0x7f) and NaN scales
    big_c = torch.full((n + 96, E), 0x7F, dtype=torch.uint8, device=dev)
    big_s = torch.full((n + 96,), float("nan"), dtype=torch.float32, device=dev)
    big_c[32: 32 + n] = cd
    big_s[32: 32 + n] = sd
    vc, vs = big_c[32: 32 + n], big_s[32: 32 + n]
    assert vc.is_contiguous() and vc.data_ptr() == big_c.data_ptr() + 32 * E
    s, r = ops.ivf_scan_fp8(qd, vc, vs, lbd, pd, k)
    assert bool(torch.isfinite(s).all())
    assert np.array_equal(s.cpu().numpy(), ref_s) and np.array_equal(r.cpu().numpy(), ref_r)
    # the raw ABI with guard bytes around the outputs and the workspace
    L = _lib.lib()
    nlist, nprobe = lb.shape[0] - 1, probes.shape[1]
    need = L.mm_ivf_scan_fp8_workspace_bytes(n, nlist, nq, nprobe, k)
    G = 256
    out_s = torch.full((G // 4 + nq * k + G // 4,), 77.0, dtype=torch.float32, device=dev)
    out_r = torch.full((G // 8 + nq * k + G // 8,), 77, dtype=torch.int64, device=dev)
    ws = torch.full((G + need + G,), 0x5A, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(wsb):
        return L.mm_ivf_scan_fp8_fwd(qd.data_ptr(), vc.data_ptr(), vs.data_ptr(), lbd.data_ptr(), pd.data_ptr(), n, nlist, nq,
                                     nprobe, E, _lib.MM_F16, k, out_s.data_ptr() + G, out_r.data_ptr() + G, ws.data_ptr() + G,
                                     wsb, stream)

    assert call(need - 1) == _lib.MM_EWORKSPACE                            # one byte less: refused, nothing written
    torch.cuda.synchronize(dev)
    assert bool((out_s == 77.0).all()) and bool((out_r == 77).all()) and bool((ws == 0x5A).all())
    assert call(need) == _lib.MM_OK
    torch.cuda.synchronize(dev)
    assert bool((out_s[: G // 4] == 77.0).all()) and bool((out_s[-(G // 4):] == 77.0).all())
    assert bool((out_r[: G // 8] == 77).all()) and bool((out_r[-(G // 8):] == 77).all())
    assert bool((ws[:G] == 0x5A).all()) and bool((ws[-G:] == 0x5A).all())
    assert np.array_equal(out_s[G // 4: G // 4 + nq * k].view(nq, k).cpu().numpy(), ref_s)
    assert np.array_equal(out_r[G // 8: G // 8 + nq * k].view(nq, k).cpu().numpy(), ref_r)


# ---- 5. random unit rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("E", [128, 768])
def test_random_unit_rows_stay_within_the_derived_bound(dtype, E):
    k = 100
    q, codes, scales, lb, probes = I8.random_problem(dtype, E)
    s, r = _scan(q, codes, scales, lb, probes, k, getattr(torch, dtype))
    worst = I8.check_union_within_bound(q, codes, scales, lb, probes, k, s, r)
    print(f"ivf_scan_fp8 random unit rows {dtype} E {E}: worst |error| / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- 6. reproducibility ------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal_and_a_query_does_not_depend_on_its_batch():
    from matchmaker_amd import ops
    q, codes, scales, lb, probes = I8.random_problem("float16", 128, nq=257)
    qd, cd, sd, lbd, pd = _dev(q, codes, scales, lb, probes)
    qd = qd.half()
    s0, r0 = ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, 100)
    s1, r1 = ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, 100)
    assert torch.equal(s0, s1) and torch.equal(r0, r1)
    s2, r2 = ops.ivf_scan_fp8(qd[:1], cd, sd, lbd, pd[:1], 100)
    assert torch.equal(s2[0], s0[0]) and torch.equal(r2[0], r0[0])


# ---- 7. graph replay -----------------------------------------------------------------------------------------------------------
def test_graph_replay_is_bit_equal_to_the_eager_call():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, codes, scales, lb, probes = I8.random_problem("float16", 384, nq=64)
    qd, cd, sd, lbd, pd = _dev(q, codes, scales, lb, probes)
    qd = qd.half()
    es, er = ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, 100)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, 100)              # warm-up on the capture stream's side
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gr = ops.ivf_scan_fp8(qd, cd, sd, lbd, pd, 100)
    gs.zero_()
    gr.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(gs, es) and torch.equal(gr, er)


# ---- 8. the indexer with every list probed -------------------------------------------------------------------------------------
def test_indexer_probing_every_list_equals_the_flat_fp8_search_bit_for_bit():
    from matchmaker_amd import ops
    from matchmaker_amd.retrieval import IVFFp8IPIndexer
    dev = util.require_gpu()
    N, E, k = 5000, 128, 50
    q, codes, scales = R.scaled_store(20, N, E, 31)
    qd, cd, sd = _dev(q, codes, scales)
    qd = qd.half()
    ix = IVFFp8IPIndexer({"token_dim": E, "faiss_ivf_list_count": 16, "faiss_ivf_search_probe_count": 16}, device=dev)
    ix.train_codes(cd, sd)
    ix.index_codes(torch.arange(N, device=dev), cd, sd)
    assert int(ix.list_begin[-1]) == N and torch.equal(ix.codes, cd[ix.ids]) and torch.equal(ix.scales, sd[ix.ids])
    s, ids = ix.search_device(qd, k + 1)                        # (one more: the right-hand neighbour of position k - 1)
    fs, fi = ops.dot_topk_fp8(qd, cd, sd, k + 1)
    assert torch.equal(s, fs)
    s = s.cpu().numpy()
    clear = np.ones((s.shape[0], k), bool)                      # positions whose score differs from both neighbours
    clear &= np.diff(s, axis=1) != 0
    clear[:, 1:] &= np.diff(s, axis=1)[:, : k - 1] != 0
    assert clear.any()
    assert (ids.cpu().numpy()[:, :k][clear] == fi.cpu().numpy()[:, :k][clear]).all()


# ---- 9. the indexer against the restatement ------------------------------------------------------------------------------------
def test_indexer_against_the_restatement_and_bit_equal_builds():
    from matchmaker_amd import ops
    from matchmaker_amd.retrieval import IVFFp8IPIndexer
    dev = util.require_gpu()
    n, E, nlist, k = 30000, 128, 200, 100
    x, centres = IR.clustered(n, E, nlist, 21, spread=1.0)
    ids = torch.arange(n, dtype=torch.int64, device=dev) * 2 + 1
    xd = torch.from_numpy(x).to(dev)
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": 5}
    a = IVFFp8IPIndexer(cfg, device=dev, native_kmeans=True)
    a.train_resident(xd)
    a.index_resident(ids, xd)
    b = IVFFp8IPIndexer(cfg, device=dev, native_kmeans=True)   # the same seed, filled through the other door
    b.train_resident(xd)
    b.index_codes(ids, *ops.fp8_quantize_rows(xd))
    for f in ("centroids", "codes", "scales", "ids", "list_begin"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    rng = np.random.default_rng(22)
    qv = (centres[rng.integers(0, nlist, 40)] + 1.0 / np.sqrt(E) * rng.standard_normal((40, E))).astype(np.float32)
    s, got_ids, probes = a.search_device(qv, k, return_probes=True)
    codes, scales, lb = a.codes.cpu().numpy(), a.scales.cpu().numpy(), a.list_begin.cpu().numpy()
    row_of = np.full(2 * n + 2, -1, np.int64)
    row_of[a.ids.cpu().numpy()] = np.arange(n)
    got_ids = got_ids.cpu().numpy()
    rows = np.where(got_ids >= 0, row_of[np.maximum(got_ids, 0)], -1)
    q16 = qv.astype(np.float16).astype(np.float32)
    worst = I8.check_union_within_bound(q16, codes, scales, lb, probes.cpu().numpy(), k, s.cpu().numpy(), rows)
    print(f"IVFFp8IPIndexer clustered 30000 x 128, nlist 200, nprobe 5: worst |error| / bound = {worst:.4f}")
    assert worst <= 1.0
    assert np.array_equal(F.dequantize_numpy(codes, scales).astype(np.float16),
                          F.dequantize_torch(*F.quantize_torch(torch.from_numpy(x)), torch.float16).numpy()[(a.ids.cpu().numpy() - 1) // 2])


# ---- 10. end to end on an fp8-ONLY store -----------------------------------------------------------------------------------------
def test_fp8_only_store_retrieves_end_to_end_through_its_token_index():
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import IVFFp8IPIndexer
    from matchmaker_amd.token_store import TokenStore
    dev = util.require_gpu()
    tokens, q, begin, end = I8.normal_store()
    st = TokenStore(tokens.to(dev), list(range(len(begin))), begin, end).quantize_fp8()      # no kept tokens
    with pytest.raises(NativeError):
        st.tokens
    ix = st.build_token_index({"faiss_ivf_list_count": 8, "faiss_ivf_search_probe_count": 8})
    assert type(ix) is IVFFp8IPIndexer and sorted(ix.ids.tolist()) == list(range(tokens.shape[0]))
    k = I8.NORMAL_K
    qd = q.to(dev)
    ivf_hits = st.token_hits(qd, k, index=ix)
    flat_hits = st.token_hits(qd, k, token_search="fp8")
    k_sorted = lambda h: torch.sort(h.view(-1, k), dim=1).values           # the same rows per token (the kernels sum in another order)
    assert torch.equal(k_sorted(ivf_hits), k_sorted(flat_hits))
    s0, d0 = st.search_device(qd, 50, k, token_search="fp8")
    s1, d1 = st.search_device(qd, 50, k, index=ix, query_chunk=40)
    assert torch.equal(s0, s1) and torch.equal(d0, d1) and bool((d0[:, 0] >= 0).all())
