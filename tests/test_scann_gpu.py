"""GPU tests of the quantized index: ops.ah_encode / ops.ah_scan / ops.gather_dot (mm_ah_encode, mm_ah_scan_fwd,
mm_gather_dot) and ScannIPIndexer against the numpy restatement in tests/scann_reference.py.  Acceptance of a scan result
= test_ivf_gpu._check_union's, with the probe score of a row's list added to its score."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_reference as IR
from tests import scann_reference as SR
from tests import util
from tests.test_ivf_gpu import LENS

pytestmark = pytest.mark.gpu

EXACT_N, EXACT_NLIST, EXACT_SEED = 37, 5, 7


def eta_of(E, T=0.2):
    return (E - 1) * T * T / (1 - T * T)


def _tol(E):
    return util.TOL_BF16 if E <= 256 else 5e-2


def _check_union(q, dec, lb, probes, pscores, k, s, rows, tol):
    """q, dec: fp32 / fp64 numpy of the 16-bit values the device saw (dec = the decoded codes)"""
    nq = q.shape[0]
    assert s.shape == (nq, k) and rows.shape == (nq, k)
    for r in range(nq):
        union, add = SR.union_scores(lb, probes[r], pscores[r])
        kk = min(k, union.size)
        if kk < k:
            assert (rows[r, kk:] == -1).all() and np.isneginf(s[r, kk:]).all(), r
        if kk == 0:
            continue
        got_rows = rows[r, :kk]
        assert (np.diff(s[r, :kk]) <= 0).all(), r                                         # descending
        assert len(set(got_rows.tolist())) == kk and np.isin(got_rows, union).all(), r    # unique, inside the union
        full = add + dec[union].astype(np.float64) @ q[r].astype(np.float64)              # the stated formula in float64
        pos = np.searchsorted(union, got_rows)
        got = full[pos]
        np.testing.assert_allclose(s[r, :kk], got, atol=tol, rtol=1e-3)
        ref = -np.sort(-full)[:kk]
        np.testing.assert_allclose(s[r, :kk], ref, atol=tol, rtol=1e-3)
        rest = np.delete(full, pos)
        if rest.size:                                                                     # nothing left out beats the k-th
            assert rest.max() <= got[kk - 1] + 1e-3 * (1 + abs(got[kk - 1])), r


def _problem(dtype, E, nq, nprobe, seed):
    g = torch.Generator().manual_seed(seed)
    lb = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    n, nlist = int(lb[-1]), len(LENS)
    codes = torch.randint(0, 256, (n, E // 4), generator=g, dtype=torch.uint8)
    cb = torch.randn(E // 2, 16, 2, generator=g).to(dtype)
    q = torch.randn(nq, E, generator=g).to(dtype)
    ps = torch.randn(nq, nprobe, generator=g)
    probes = np.stack([np.random.default_rng(seed + i).permutation(nlist)[:nprobe] for i in range(nq)]).astype(np.int32)
    # query 0 probes lists 3 (16 rows), 5 and 8 (thousands), with a hole; two rows with identical codes sit in lists 5 and
    # 8 — the codes of the highest score any row can have for query 0 — and the two lists carry one probe score
    probes[0, :4] = [8, -1, 5, 3]
    probes[0, 4:] = -1
    ps[0, :4] = torch.tensor([0.75, 9.0, 0.75, 0.5])
    a, b = int(lb[5]) + 7, int(lb[8]) + 1234
    best = (q[0].float().view(E // 2, 1, 2) * cb.float()).sum(-1).argmax(dim=1).numpy().astype(np.uint8)   # [S]
    codes[a] = torch.from_numpy(SR.pack(best[None])[0])
    codes[b] = codes[a]
    return q, codes, cb, lb, probes, ps, (a, b)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,nq,k", [(128, 1, 1), (128, 37, 10), (128, 700, 1000), (384, 1, 1000), (384, 37, 1),
                                    (384, 700, 10), (768, 1, 10), (768, 37, 1000), (768, 700, 1),
                                    (128, 3, 16), (128, 3, 4096)])      # k equal to its padded power of two; the operator's limit
def test_ah_scan_is_the_exact_topk_of_the_probed_union(dtype, E, nq, k):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, codes, cb, lb, probes, ps, (a, b) = _problem(dtype, E, nq, 6, seed=E + nq + k)
    s, rows = ops.ah_scan(q.to(dev), codes.to(dev), cb.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev),
                          ps.to(dev), k)
    s, rows = s.cpu().numpy(), rows.cpu().numpy()
    dec = SR.decode(codes.numpy(), cb.float().numpy())
    _check_union(q.float().numpy(), dec, lb, probes, ps.numpy(), k, s, rows, tol=_tol(E))
    # tie order: the planted rows score the same and lead query 0's result; the lower row comes first
    assert rows[0, 0] == a
    if k > 1:
        assert rows[0, 1] == b and s[0, 0] == s[0, 1]


def test_ah_scan_agrees_with_ivf_scan_on_the_decoded_matrix():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    E, nq, k = 384, 37, 50
    q, codes, cb, lb, probes, ps, _ = _problem(torch.float16, E, nq, 6, seed=3)
    dec = SR.decode(codes.numpy(), cb.float().numpy())
    lbd, pd = torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev)
    s, rows = ops.ah_scan(q.to(dev), codes.to(dev), cb.to(dev), lbd, pd, torch.zeros_like(ps).to(dev), k)
    vs, vrows = ops.ivf_scan(q.to(dev), torch.from_numpy(dec).to(torch.float16).to(dev), lbd, pd, k)     # 16-bit values: exact
    s, rows, vs, vrows = s.cpu().numpy(), rows.cpu().numpy(), vs.cpu().numpy(), vrows.cpu().numpy()
    np.testing.assert_allclose(s, vs, atol=_tol(E), rtol=1e-3)
    ref_s, _ = SR.ah_scan(q.float().numpy(), codes.numpy(), cb.float().numpy(), lb, probes, np.zeros_like(ps.numpy()), k + 1)
    gap = 1e-3 * (1 + np.abs(ref_s))
    clear = np.isfinite(ref_s[:, :k])                          # positions whose reference score is away from both neighbours
    with np.errstate(invalid="ignore"):
        clear &= ~((ref_s[:, :k] - ref_s[:, 1: k + 1]) <= gap[:, :k])
        clear[:, 1:] &= (ref_s[:, : k - 1] - ref_s[:, 1:k]) > gap[:, 1:k]
    print("positions with both neighbours beyond the tolerance:", round(float(clear.mean()), 4))
    assert clear[:, 0].any() and clear.mean() > 0.5
    assert (rows[clear] == vrows[clear]).all()


def test_ah_scan_k_larger_than_the_union_and_empty_rows():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, codes, cb, lb, probes, ps, _ = _problem(torch.float16, 256, 5, 4, seed=11)
    probes[:] = -1
    probes[0, :2] = [1, 2]            # 1 + 15 rows
    probes[1, 0] = 0                  # an empty list only
    probes[2, :3] = [6, 0, 4]         # empty, empty, 17
    probes[3, 2] = 12                 # 31, behind two holes
    # query 4 probes nothing at all
    k = 100
    s, rows = ops.ah_scan(q.to(dev), codes.to(dev), cb.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev),
                          ps.to(dev), k)
    s, rows = s.cpu().numpy(), rows.cpu().numpy()
    _check_union(q.float().numpy(), SR.decode(codes.numpy(), cb.float().numpy()), lb, probes, ps.numpy(), k, s, rows,
                 tol=util.TOL_BF16)
    assert [(r >= 0).sum() for r in rows] == [16, 0, 17, 31, 0]


# ---- the encoder ------------------------------------------------------------------------------------------

def plant_exact_rows(x, lists, cent, cb):
    """row 0: all zeros.  row 1: a centre of its own whose first block cancels x, so the residual (0, 0) is equally far
    from the four codewords (+-0.5, +-0.5)."""
    x, lists = x.copy(), lists.copy()
    x[0] = 0
    x[1] = 0
    x[1, 2:18] = np.where(np.arange(16) % 3 == 0, -1.0, 1.0)
    own = cent[:1].copy()
    own[0, :2] = 0
    cent = np.concatenate([cent, own])
    lists[1] = cent.shape[0] - 1
    return x, lists, cent


def _encode_on_device(x, lists, cent, cb, eta, passes, dtype=torch.float16):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)      # noqa: E731
    return ops.ah_encode(t(x), torch.from_numpy(lists).to(dev), t(cent), t(cb), eta, passes).cpu().numpy()


@pytest.mark.parametrize("E", [128, 768])
def test_ah_encode_is_bit_equal_to_the_restatement_on_an_exact_store(E):
    x, lists, cent, cb = SR.exact_store(EXACT_N, E, EXACT_NLIST, seed=EXACT_SEED)
    x, lists, cent = plant_exact_rows(x, lists, cent, cb)
    pq = SR.encode(x, lists, cent, cb, 1.0, 2)
    got = _encode_on_device(x, lists, cent, cb, 1.0, 2)
    assert got.shape == (EXACT_N, E // 4) and got.dtype == np.uint8 and (got == pq).all()
    assert (_encode_on_device(x, lists, cent, cb, eta_of(E), 0) == pq).all()          # passes = 0: plain quantisation
    # the planted equidistant block takes the lowest of its four nearest codes
    four = [k for k in range(16) if abs(cb[0, k, 0]) == 0.5 and abs(cb[0, k, 1]) == 0.5]
    assert len(four) == 4 and SR.unpack(got)[1, 0] == min(four)
    for passes in (1, 2):
        got = _encode_on_device(x, lists, cent, cb, eta_of(E), passes)
        ref = SR.encode(x, lists, cent, cb, eta_of(E), passes)
        assert (got == ref).all(), (passes, int((SR.unpack(got) != SR.unpack(ref)).sum()))
        assert (got[0] == pq[0]).all()                                                 # an all-zero row: eta counts as 1
        assert (got != pq).any()                                                       # the descent moved something
    bf = _encode_on_device(x, lists, cent, cb, eta_of(E), 2, dtype=torch.bfloat16)   # the store is exact in bfloat16 too
    assert (bf == got).all()


@functools.lru_cache(maxsize=None)
def random_encode_problem(n, E, nlist=7, seed=13):
    """float32 arrays of float16 values: near-unit rows, centres a third of their length, a codebook on the residuals' scale"""
    rng = np.random.default_rng(seed + E)
    h = lambda a: a.astype(np.float16).astype(np.float32)                              # noqa: E731
    x = h(rng.standard_normal((n, E)) / np.sqrt(E))
    cent = h(rng.standard_normal((nlist, E)) / (3 * np.sqrt(E)))
    lists = rng.integers(0, nlist, n).astype(np.int32)
    cb = h(rng.standard_normal((E // 2, 16, 2)) * 1.1 / np.sqrt(E))
    return x, lists, cent, cb


@functools.lru_cache(maxsize=None)
def _random_reference(E):
    x, lists, cent, cb = random_encode_problem(1000, E)
    ref = SR.unpack(SR.encode(x, lists, cent, cb, eta_of(E), 2))
    _, gaps = SR.encode(x, lists, cent, cb, eta_of(E), 2, dtype=np.float64, return_gaps=True)
    return ref, gaps


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
@pytest.mark.parametrize("E", [128, 768])
def test_ah_encode_on_random_data_descends_and_follows_the_restatement(E, n):
    x, lists, cent, cb = (a[:n] if i < 2 else a for i, a in enumerate(random_encode_problem(1000, E)))
    ref, gaps = _random_reference(E)
    ref, gaps = ref[:n], gaps[:n]
    eta = eta_of(E)
    got = _encode_on_device(x, lists, cent, cb, eta, 2)
    start = _encode_on_device(x, lists, cent, cb, eta, 0)
    l2, l0 = SR.loss(x, lists, cent, cb, got, eta), SR.loss(x, lists, cent, cb, start, eta)
    print(f"E {E} n {n}: mean float64 loss {l0.mean():.6f} -> {l2.mean():.6f}")
    assert (l2 <= l0 * (1 + 1e-6)).all()
    near = gaps < 1e-5
    differ = SR.unpack(got) != ref
    print(f"blocks whose two best costs are within 1e-5 relative: {int(near.sum())} of {near.size}; "
          f"blocks that differ from the float32 restatement: {int(differ.sum())}")
    assert near.sum() < 0.01 * near.size
    assert not (differ & ~near).any()


# ---- the re-score -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("E,nq,R", [(128, 1, 1), (128, 700, 33), (768, 1, 1000), (768, 700, 1), (384, 37, 33), (768, 37, 1000)])
def test_gather_dot_is_the_exact_inner_product(dtype, E, nq, R):
    from matchmaker_amd import ops
    dev = util.require_gpu()
    g = torch.Generator().manual_seed(E + nq + R)
    n = 5000
    v = torch.randn(n, E, generator=g).to(dtype)
    q = torch.randn(nq, E, generator=g).to(dtype)
    rows = torch.randint(0, n, (nq, R), generator=g)
    rows[torch.rand(nq, R, generator=g) < 0.1] = -1
    rows[0, 0] = -1
    if R > 2:
        rows[:, 2] = rows[:, 1]                                    # repeated rows
        rows[-1, -1] = n - 1
    out = ops.gather_dot(q.to(dev), v.to(dev), rows.to(dev)).cpu().numpy()
    ref = SR.gather_dot(q.float().numpy(), v.float().numpy(), rows.numpy())
    hole = rows.numpy() < 0
    assert out.shape == (nq, R) and np.isneginf(out[hole]).all() and np.isfinite(out[~hole]).all()
    np.testing.assert_allclose(out[~hole], ref[~hole], atol=_tol(E), rtol=1e-3)
    if R > 2:
        assert (out[:, 2] == out[:, 1]).all()


# ---- the indexer ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clustered():
    """test_ivf_gpu._clustered_index's collection: 30,000 x 128, int(sqrt(30000)) = 173 leaves, every leaf probed"""
    from matchmaker_amd.retrieval import FlatIPIndexer, ScannIPIndexer
    dev = util.require_gpu()
    n, E, seed = 30000, 128, 21
    x, centres = IR.clustered(n, E, 200, seed, spread=1.0)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    cfg = {"token_dim": E, "token_dtype": "float16", "query_sets": {"dev": {"top_n": 100}}, "scann_leaves_to_search": 173}
    ix = ScannIPIndexer(cfg, device=dev)
    ix.index([ids], [x])
    flat = FlatIPIndexer(cfg, device=dev)
    flat.index([ids], [x])
    rng = np.random.default_rng(seed + 1)
    qv = (centres[rng.integers(0, 200, 300)] + 1.0 / np.sqrt(E) * rng.standard_normal((300, E))).astype(np.float32)
    ref = qv.astype(np.float16).astype(np.float64) @ x.astype(np.float64).T
    return ix, flat, x, ids, qv, ref, cfg, dev


def test_full_probe_and_the_largest_reorder_equal_the_flat_index(clustered):
    """Every leaf probed makes the union the whole collection (30,000 rows); the scan returns at most 4,096 candidates, so
    the reorder count is that maximum rather than the size of the union."""
    ix, flat, x, ids, qv, ref, _, _ = clustered
    assert ix.nlist == 173 and ix.leaves_to_search == 173
    ix.reorder = 4096
    k = 50
    s, i = ix.search(qv, k)
    fs, fi = flat.search(qv, k)
    ref_s = -np.sort(-ref, axis=1)[:, : k + 1]
    gap = 1e-3 * (1 + np.abs(ref_s))
    clear = np.ones((qv.shape[0], k), bool)
    clear &= (ref_s[:, :k] - ref_s[:, 1: k + 1]) > gap[:, :k]
    clear[:, 1:] &= (ref_s[:, : k - 1] - ref_s[:, 1:k]) > gap[:, 1:k]
    print("positions with both neighbours beyond the tolerance:", round(float(clear.mean()), 4))
    assert clear[:, 0].any()
    assert (i[clear] == fi[clear]).all()
    np.testing.assert_allclose(s, fs, atol=util.TOL_BF16, rtol=1e-3)
    # returned scores are the exact inner products of the returned ids
    np.testing.assert_allclose(s, np.take_along_axis(ref, (i - 1) // 2, 1), atol=util.TOL_BF16, rtol=1e-3)


def test_recall_does_not_fall_with_the_reorder_count(clustered):
    ix, flat, x, ids, qv, ref, _, _ = clustered
    k = 100
    _, fi = flat.search(qv, k)
    kth = np.take_along_axis(ref, (fi - 1) // 2, 1).min(axis=1)
    tol = 1e-3 * (1 + np.abs(kth))
    recalls = []
    for reorder in (100, 400, 4096):
        ix.reorder = reorder
        s, i = ix.search(qv, k)
        assert all(len(set(r)) == k for r in i.tolist())
        got = np.take_along_axis(ref, (i - 1) // 2, 1)
        np.testing.assert_allclose(s, got, atol=util.TOL_BF16, rtol=1e-3)      # exact scores at every reorder count
        # an id outside the flat set counts as found when it reaches the k-th flat score within the tolerance: candidates
        # that tie at the cut may swap between two kernels that sum in different orders
        hit = np.array([[e in f for e in row] for row, f in zip(i.tolist(), map(set, fi.tolist()))]) | (got >= (kth - tol)[:, None])
        recalls.append(float(hit.mean()))
    print("recall@100 against flat for reorder 100, 400, 4096 (every leaf probed):", [round(r, 4) for r in recalls])
    assert all(b >= a for a, b in zip(recalls, recalls[1:])), recalls
    assert recalls[0] > 0.5


def test_two_builds_from_one_seed_are_bit_equal(clustered):
    from matchmaker_amd.retrieval import ScannIPIndexer
    ix, _, x, ids, _, _, cfg, dev = clustered
    again = ScannIPIndexer(cfg, device=dev)
    again.index([ids], [x])
    for name in ("centroids", "codebook", "codes", "vectors", "ids", "list_begin"):
        assert torch.equal(getattr(again, name), getattr(ix, name)), name
    lb = ix.list_begin.cpu().numpy()
    assert lb[0] == 0 and lb[-1] == x.shape[0] and ix.codes.shape == (x.shape[0], 32)


def test_graph_replay_is_bit_equal_to_the_eager_call():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    q, codes, cb, lb, probes, ps, _ = _problem(torch.float16, 384, 64, 6, seed=5)
    v = torch.randn(codes.shape[0], 384, generator=torch.Generator().manual_seed(6)).half().to(dev)
    qd, cd, cbd, lbd, pd, psd = q.to(dev), codes.to(dev), cb.to(dev), torch.from_numpy(lb).to(dev), torch.from_numpy(probes).to(dev), ps.to(dev)

    def run():
        s, r = ops.ah_scan(qd, cd, cbd, lbd, pd, psd, 100)
        return s, r, ops.gather_dot(qd, v, r)

    es, er, ee = run()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run()                                                   # warm-up on the capture stream's side
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gs, gr, ge = run()
    gs.zero_()
    gr.zero_()
    ge.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(gs, es) and torch.equal(gr, er) and torch.equal(ge, ee)
