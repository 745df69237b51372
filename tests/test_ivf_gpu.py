"""GPU tests of the IVF list scan (ops.ivf_scan = mm_ivf_scan_fwd) and of IVFFlatIPIndexer against the numpy
restatement in tests/ivf_reference.py.  Acceptance of a scan result = test_dot_topk_gpu._check, over the union of
the probed lists instead of the whole collection."""
import numpy as np
import pytest
import torch

from tests import ivf_reference as IR
from tests import util

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 3000, 0, 33, 5000, 64, 2500, 100, 31, 32, 4097]


def _check_union(q, v, lb, probes, k, s, rows, tol):
    """q, v: fp32 numpy of the 16-bit values the device saw"""
    nq = q.shape[0]
    assert s.shape == (nq, k) and rows.shape == (nq, k)
    ref_s, _ = IR.ivf_scan(q, v, lb, probes, k)
    for r in range(nq):
        union = IR.union_rows(lb, probes[r])
        kk = min(k, union.size)
        if kk < k:
            assert (rows[r, kk:] == -1).all() and np.isneginf(s[r, kk:]).all(), r
        if kk == 0:
            continue
        got_rows = rows[r, :kk]
        # descending, valid, unique, inside the probed lists
        assert (np.diff(s[r, :kk]) <= 0).all(), r
        assert len(set(got_rows.tolist())) == kk and np.isin(got_rows, union).all(), r
        # reported scores are the true inner products
        full = v[union].astype(np.float64) @ q[r].astype(np.float64)
        got = v[got_rows].astype(np.float64) @ q[r].astype(np.float64)
        np.testing.assert_allclose(s[r, :kk], got, atol=tol, rtol=1e-3)
        np.testing.assert_allclose(s[r, :kk], ref_s[r, :kk], atol=tol, rtol=1e-3)
        # exactness of the set: nothing else in the union beats the k-th returned score beyond the accumulation noise
        rest = full[~np.isin(union, got_rows)]
        if rest.size:
            assert rest.max() <= got[kk - 1] + 1e-3 * (1 + abs(got[kk - 1])), r


def _problem(dtype, E, nq, nprobe, seed):
    g = torch.Generator().manual_seed(seed)
    lb = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    n, nlist = int(lb[-1]), len(LENS)
    v = torch.randn(n, E, generator=g).to(dtype)
    q = torch.randn(nq, E, generator=g).to(dtype)
    probes = np.stack([np.random.default_rng(seed + i).permutation(nlist)[:nprobe] for i in range(nq)]).astype(np.int32)
    # query 0 probes lists 3 (16 rows), 5 and 8 (thousands), with a hole; two exact copies of one vector sit in lists 5 and 8
    probes[0, :4] = [8, -1, 5, 3]
    probes[0, 4:] = -1
    a, b = int(lb[5]) + 7, int(lb[8]) + 1234
    v[a] = (q[0].float() * 1.5).to(dtype)
    v[b] = v[a]
    return q, v, lb, probes, (a, b)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,nq,k", [(128, 1, 1), (128, 37, 10), (128, 700, 1000), (384, 1, 1000), (384, 37, 1),
                                    (384, 700, 10), (768, 1, 10), (768, 37, 1000), (768, 700, 1),
                                    (128, 3, 16), (128, 3, 4096)])      # k equal to its padded power of two; the operator's limit
def test_ivf_scan_is_the_exact_topk_of_the_probed_union(dtype, E, nq, k):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, v, lb, probes, (a, b) = _problem(dtype, E, nq, 6, seed=E + nq + k)
    s, rows = ops.ivf_scan(q.to(dev), v.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev), k)
    s, rows = s.cpu().numpy(), rows.cpu().numpy()
    _check_union(q.float().numpy(), v.float().numpy(), lb, probes, k, s, rows, tol=util.TOL_BF16 if E <= 256 else 5e-2)
    # tie order: the planted copies score the same and lead query 0's result; the lower row comes first
    assert rows[0, 0] == a
    if k > 1:
        assert rows[0, 1] == b and s[0, 0] == s[0, 1]


def test_ivf_scan_k_larger_than_the_union_and_empty_rows():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, v, lb, probes, _ = _problem(torch.float16, 256, 5, 4, seed=11)
    probes[:] = -1
    probes[0, :2] = [1, 2]            # 1 + 15 vectors
    probes[1, 0] = 0                  # an empty list only
    probes[2, :3] = [6, 0, 4]         # empty, empty, 17
    probes[3, 2] = 12                 # 31, behind two holes
    # query 4 probes nothing at all
    k = 100
    s, rows = ops.ivf_scan(q.to(dev), v.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev), k)
    s, rows = s.cpu().numpy(), rows.cpu().numpy()
    _check_union(q.float().numpy(), v.float().numpy(), lb, probes, k, s, rows, tol=util.TOL_BF16)
    assert [(r >= 0).sum() for r in rows] == [16, 0, 17, 31, 0]


def _scan_exact(q, v, lb, probes, k):
    """the fp16 scan of an integer-valued problem (exact in fp16 and in any fp32 summation order) -> numpy scores, rows"""
    from matchmaker_amd import ops
    dev = util.require_gpu()
    s, rows = ops.ivf_scan(torch.from_numpy(q).half().to(dev), torch.from_numpy(v).half().to(dev), torch.from_numpy(lb).to(dev),
                           torch.from_numpy(probes).to(dev), k)
    return s.cpu().numpy(), rows.cpu().numpy()


def test_block_scans_carry_past_their_1024_thread_tile_bit_for_bit():
    """1,030 lists and 1,030 queries: ivf_tasks_kernel, ivf_lscan_kernel (over the lists) and ivf_chunks_kernel (over the
    queries) each scan one tile of 1,024 and carry into a second one, whose lists and queries are probed and answered."""
    q, v, lb, probes, k = IR.carry_problem()
    s, rows = _scan_exact(q, v, lb, probes, k)
    ref_s, ref_r = IR.ivf_scan(q, v, lb, probes, k)
    assert np.array_equal(rows, ref_r), f"rows differ for queries {np.nonzero((rows != ref_r).any(axis=1))[0][:10]}"
    assert np.array_equal(s, ref_s.astype(np.float32))                     # (-inf pads compare equal)
    assert (rows[1024:, 0] >= lb[1024]).any()                               # rows of the lists behind the tile are returned


def test_more_ties_at_the_kth_score_than_fit_keep_the_lowest_rows():
    """40 bit-identical rows over two probed lists tie from rank 8 on, k = 10: the second radix selection (over the row
    numbers of the candidates that tie with the k-th score) keeps the three lowest rows of the group."""
    q, v, lb, probes, k, group = IR.tie_problem()
    s, rows = _scan_exact(q, v, lb, probes, k)
    ref_s, ref_r = IR.ivf_scan(q, v, lb, probes, k)
    assert np.array_equal(rows, ref_r) and np.array_equal(s, ref_s.astype(np.float32))
    assert rows[0, 7:].tolist() == group[:3].tolist() and (s[0, 7:] == s[0, 7]).all() and s[0, 6] > s[0, 7]


def _clustered_index(dev, n=30000, E=128, nlist=200, nprobe=5, seed=21):
    from matchmaker_amd.retrieval import FlatIPIndexer, IVFFlatIPIndexer
    x, centres = IR.clustered(n, E, nlist, seed, spread=1.0)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": nprobe}
    ivf = IVFFlatIPIndexer(cfg, device=dev)
    ivf.prepare([x])
    ivf.index([ids], [x])
    flat = FlatIPIndexer(cfg, device=dev)
    flat.index([ids], [x])
    rng = np.random.default_rng(seed + 1)
    qv = centres[rng.integers(0, nlist, 300)] + 1.0 / np.sqrt(E) * rng.standard_normal((300, E))
    return ivf, flat, x, ids, qv.astype(np.float32)


def test_probing_every_list_equals_the_flat_index():
    dev = util.require_gpu()
    ivf, flat, x, ids, qv = _clustered_index(dev)
    ivf.nprobe = ivf.nlist
    k = 50
    s, i = ivf.search(qv, k)
    fs, fi = flat.search(qv, k)
    np.testing.assert_allclose(s, fs, atol=util.TOL_BF16, rtol=1e-3)
    ref = qv.astype(np.float16).astype(np.float64) @ x.astype(np.float64).T
    ref_s = -np.sort(-ref, axis=1)[:, : k + 1]
    gap = 1e-3 * (1 + np.abs(ref_s))
    clear = np.ones((qv.shape[0], k), bool)                     # positions whose reference score is away from both neighbours
    clear &= (ref_s[:, :k] - ref_s[:, 1: k + 1]) > gap[:, :k]
    clear[:, 1:] &= (ref_s[:, : k - 1] - ref_s[:, 1:k]) > gap[:, 1:k]
    print("positions with both neighbours beyond the tolerance:", round(float(clear.mean()), 4))
    assert clear[:, 0].any()                                    # the check below is not empty
    assert (i[clear] == fi[clear]).all()


def test_recall_grows_with_nprobe_and_reaches_one():
    dev = util.require_gpu()
    ivf, flat, x, ids, qv = _clustered_index(dev)
    k = 100
    _, fi = flat.search(qv, k)
    recalls = []
    for nprobe in (1, 2, 5, 20, 80, ivf.nlist):
        ivf.nprobe = nprobe
        _, i = ivf.search(qv, k)
        recalls.append(np.mean([len(set(a) & set(b)) / k for a, b in zip(i.tolist(), fi.tolist())]))
    print("recall@100 for nprobe 1, 2, 5 (2.5 % of the lists), 20, 80, all:", [round(r, 4) for r in recalls])
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    # at nprobe = nlist the candidate set is the whole collection: recall is 1.  The two kernels sum in different orders, so
    # candidates that tie AT THE CUT may swap: an id outside the flat set counts as found only when it replaces a flat id
    # whose float64 score is itself within the scan test's tolerance of the k-th score, and reaches that score within the
    # same tolerance.  Anything that scores clearly above the cut must be in both sets.
    ref = qv.astype(np.float16).astype(np.float64) @ x.astype(np.float64).T
    swaps = 0
    for r, (a, b) in enumerate(zip(i.tolist(), fi.tolist())):
        kth = ref[r, (np.array(b) - 1) // 2].min()
        tol = 1e-3 * (1 + abs(kth))
        extra, missing = set(a) - set(b), set(b) - set(a)
        assert len(set(a)) == k and len(extra) == len(missing), r
        assert all(ref[r, (e - 1) // 2] >= kth - tol for e in extra), r
        assert all(ref[r, (e - 1) // 2] <= kth + tol for e in missing), r
        swaps += len(extra)
    print("ids swapped at the cut:", swaps, "of", k * qv.shape[0])


def test_every_vector_sits_in_the_list_of_its_best_centroid():
    dev = util.require_gpu()
    ivf, _, x, ids, _ = _clustered_index(dev)
    lb = ivf.list_begin.cpu().numpy()
    v = ivf.vectors.float().cpu().numpy().astype(np.float64)
    cent = ivf.centroids.float().cpu().numpy().astype(np.float64)
    assert lb[0] == 0 and lb[-1] == v.shape[0] and (np.diff(lb) >= 0).all()
    stored = np.repeat(np.arange(ivf.nlist), np.diff(lb))
    sc = v @ cent.T
    best = sc.max(axis=1)
    mine = sc[np.arange(v.shape[0]), stored]
    assert (mine >= best - 1e-3 * (1 + np.abs(best))).all()      # never worse than a near-tie
    near = int((stored != sc.argmax(axis=1)).sum())
    print("vectors stored in a near-tie list:", near, "of", v.shape[0])
    assert near < 0.01 * v.shape[0]
    assert (ivf.ids.cpu().numpy() == ids[(ivf.ids.cpu().numpy() - 1) // 2]).all()
    assert (v[:, :128] == x.astype(np.float64)[(ivf.ids.cpu().numpy() - 1) // 2]).all()


def test_graph_replay_is_bit_equal_to_the_eager_call():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, v, lb, probes, _ = _problem(torch.float16, 384, 64, 6, seed=5)
    qd, vd, lbd, pd = q.to(dev), v.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev)
    es, er = ops.ivf_scan(qd, vd, lbd, pd, 100)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.ivf_scan(qd, vd, lbd, pd, 100)                      # warm-up on the capture stream's side
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gr = ops.ivf_scan(qd, vd, lbd, pd, 100)
    gs.zero_()
    gr.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(gs, es) and torch.equal(gr, er)
