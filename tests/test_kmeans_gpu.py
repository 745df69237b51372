"""GPU tests of mm_kmeans_assign / mm_kmeans_segment_sum (called with outputs and workspace pre-filled with NaN), of
spherical_kmeans, DynamicIVFIndexer and IVFFlatIPIndexer(native_kmeans=True) against the float64 numpy restatement in
tests/kmeans_reference.py.

Exact store: values that are multiples of 1/4 in [-2, 2] make every product and every partial sum exact in fp32 in any
order, so the device must reproduce the float64 results bit for bit, ties included.
Ordinary data: products of 16-bit values are exact in fp32 and (E - 1) 2^-24 sum_i |x_i c_i| bounds one fp32 accumulation
in any order; the margin a row needs to be DECIDED doubles that for the two scores compared and doubles it again because
the MFMA's internal rounding is not specified per addition: 4 E 2^-24 max_c sum_i |x_i c_i|."""
import functools

import numpy as np
import pytest
import torch

from tests import ivf_reference as IR
from tests import kmeans_reference as KR
from tests import util

pytestmark = pytest.mark.gpu

TORCH_DT = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def _padded(a, E_pad):
    out = np.zeros((a.shape[0], E_pad), np.float32)
    out[:, : a.shape[1]] = a
    return out


def _dev(a, dev, dtype=torch.float16):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).to(dtype)


def _assign(x, c):
    """mm_kmeans_assign on device tensors, outputs pre-filled (-1, NaN)"""
    from matchmaker_amd import _lib, ops
    n, E = x.shape
    out_l = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    out_s = torch.full((n,), float("nan"), dtype=torch.float32, device=x.device)
    rc = _lib.lib().mm_kmeans_assign(x.data_ptr() if n else None, c.data_ptr(), n, c.shape[0], E, ops._DT[x.dtype],
                                     out_l.data_ptr(), out_s.data_ptr(), ops._stream(x.device))
    _lib.check(rc, "mm_kmeans_assign")
    torch.cuda.synchronize(x.device)
    return out_l.cpu().numpy(), out_s.cpu().numpy()


def _segment_sum(x, order, lb):
    """mm_kmeans_segment_sum on device tensors, sums and workspace pre-filled with NaN"""
    from matchmaker_amd import _lib, ops
    n, E = x.shape
    nlist = lb.shape[0] - 1
    L = _lib.lib()
    wsb = L.mm_kmeans_segment_sum_workspace_bytes(n, nlist, E)
    assert wsb % 4 == 0 and wsb > 0
    ws = torch.full((wsb // 4,), float("nan"), dtype=torch.float32, device=x.device)
    sums = torch.full((nlist, E), float("nan"), dtype=torch.float32, device=x.device)
    rc = L.mm_kmeans_segment_sum(x.data_ptr(), order.data_ptr(), lb.data_ptr(), n, nlist, E, ops._DT[x.dtype], sums.data_ptr(),
                                 ws.data_ptr(), wsb, ops._stream(x.device))
    _lib.check(rc, "mm_kmeans_segment_sum")
    torch.cuda.synchronize(x.device)
    return sums.cpu().numpy()


def _i64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


# ---- exact store ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_problem(n, E, nlist, seed=11):
    x = KR.exact_store(n, E, seed)
    c = KR.exact_store(nlist, E, seed + 1)
    if nlist == 37:
        c[20] = c[5]
        c[36] = c[0]
    if n > 1:
        x[n // 2] = 0                                           # an all-zero row: every score ties at 0
    a, s = KR.assign(x, c)
    for t in (x, c, a, s):
        t.setflags(write=False)
    return x, c, a, s


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_exact_store_assignment_is_bit_equal_and_copies_never_win(dtype):
    dev = util.require_gpu()
    x, c, a, s = _exact_problem(1999, 128, 37)
    assert np.abs(s).max() < 512 and (s * 16 == np.round(s * 16)).all()
    got_l, got_s = _assign(_dev(x, dev, TORCH_DT[dtype]), _dev(c, dev, TORCH_DT[dtype]))
    assert got_l.dtype == np.int32 and got_s.dtype == np.float32
    assert (got_l == a).all()
    assert (got_s.astype(np.float64) == s).all()
    assert not np.isin(got_l, (20, 36)).any()
    assert got_l[1999 // 2] == 0 and got_s[1999 // 2] == 0


@pytest.mark.parametrize("n,E,nlist", [(300, 768, 33), (300, 128, 1), (300, 128, 130), (300, 128, 1025), (1, 128, 37),
                                       (300, 256, 33), (300, 384, 65), (300, 512, 33)])
def test_assignment_shapes_on_the_exact_store(n, E, nlist):
    dev = util.require_gpu()
    x, c, a, s = _exact_problem(n, E, nlist)
    got_l, got_s = _assign(_dev(x, dev), _dev(c, dev))
    assert (got_l == a).all()
    assert (got_s.astype(np.float64) == s).all()


def test_no_rows_and_padded_width():
    from matchmaker_amd import ops
    from matchmaker_amd.retrieval import DynamicIVFIndexer
    dev = util.require_gpu()
    x, c, a, s = _exact_problem(300, 96, 37)
    got_l, got_s = _assign(_dev(x[:0], dev).reshape(0, 128), _dev(_padded(c, 128), dev))      # success without a launch
    assert got_l.shape == (0,) and got_s.shape == (0,)
    l0, s0 = ops.kmeans_assign(torch.zeros((0, 128), dtype=torch.float16, device=dev), _dev(_padded(c, 128), dev))
    assert l0.shape == (0,) and l0.dtype == torch.int32 and s0.shape == (0,) and s0.dtype == torch.float32
    # E = 96 through the index's padding
    ix = DynamicIVFIndexer({"token_dim": 96, "faiss_ivf_list_count": 37}, device=dev)
    ix.centroids = _dev(_padded(c, 128), dev)
    got = ix.assign(x.copy())
    assert got.dtype == torch.int64 and (got.cpu().numpy() == a).all()
    l1, s1 = ops.kmeans_assign(_dev(_padded(x, 128), dev), ix.centroids)
    assert (l1.cpu().numpy() == a).all() and (s1.cpu().numpy().astype(np.float64) == s).all()


# ---- ordinary data ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,E,clusters,nlist", [(3000, 128, 40, 37), (2500, 768, 40, 33), (5000, 96, 50, 130)])
def test_ordinary_data_decided_rows_match_and_the_rest_are_near_ties(n, E, clusters, nlist):
    dev = util.require_gpu()
    x, _ = IR.clustered(n, E, clusters, seed=5)
    c = IR.spherical_kmeans(x, nlist, iters=3, seed=1)
    x32, c32 = x.astype(np.float32), c.astype(np.float32)
    margin, absdot, s = KR.margin_and_bound(x32, c32)
    thr = 4 * E * 2.0 ** -24 * absdot
    decided = margin > thr
    print(f"undecided rows: {int((~decided).sum())} of {n}; min margin {margin.min():.3g}, max threshold {thr.max():.3g}")
    assert (~decided).sum() <= 0.01 * n                         # the cap holds on the reference itself
    E_pad = 128 if E <= 128 else E
    got_l, got_s = _assign(_dev(_padded(x32, E_pad), dev), _dev(_padded(c32, E_pad), dev))
    ref = s.argmax(axis=1)
    assert (got_l >= 0).all() and (got_l < nlist).all()
    assert (got_l[decided] == ref[decided]).all()
    best = s.max(axis=1)
    assert (s[np.arange(n), got_l] >= best - thr).all()
    assert (np.abs(got_s - s[np.arange(n), got_l]) <= thr).all()


# ---- segment sums -----------------------------------------------------------------------------------------------------

def _check_exact_sums(dev, x, order, lb, dtype=torch.float16):
    got = _segment_sum(_dev(x, dev, dtype), _i64(order, dev), _i64(lb, dev))
    ref = KR.segment_sum(x, order, lb)
    assert got.dtype == np.float32 and not np.isnan(got).any()
    assert (got.astype(np.float64) == ref).all()
    return got


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_exact_store_segment_sums_of_the_assignment(dtype):
    dev = util.require_gpu()
    x, c, a, _ = _exact_problem(1999, 128, 37)
    # 300 lists: lists of one row and empty lists occur
    a = (a * 8 + np.arange(1999) % 8) * 300 // (37 * 8)
    a[7] = 299
    order, lb = KR.lists_of(a, 300)
    assert (np.diff(lb) == 1).any() and (np.diff(lb) == 0).any()
    _check_exact_sums(dev, x, order, lb, TORCH_DT[dtype])
    order, lb = KR.lists_of(_exact_problem(1999, 128, 37)[2], 37)
    _check_exact_sums(dev, x, order, lb, TORCH_DT[dtype])


@pytest.mark.parametrize("E", [128, 384, 768])
def test_exact_store_segment_sums_empty_lists_long_list_and_one_list(E):
    dev = util.require_gpu()
    n = 5000 if E == 128 else 1500
    x = KR.exact_store(n, E, seed=3)
    perm = np.random.default_rng(4).permutation(n).astype(np.int64)
    # empty lists at the start, in the middle and at the end; a list of exactly one chunk, and one a row longer
    lb = np.array([0, 0, 0, 512, 512, 1025, 1025, 1400, n, n, n], np.int64)
    _check_exact_sums(dev, x, perm, lb)
    # every row in one list of several lists (crosses the chunk split), and nlist = 1
    _check_exact_sums(dev, x, perm, np.array([0, 0, n, n], np.int64))
    _check_exact_sums(dev, x, perm, np.array([0, n], np.int64))
    # rows outside [0, n) are skipped, not read
    bad = perm.copy()
    bad[[0, 17, 600, n - 1]] = [-1, n, n + 12345, -(2 ** 40)]
    _check_exact_sums(dev, x, bad, lb)
    # a list_begin that stops short of n: the rest of `order` belongs to no list
    _check_exact_sums(dev, x, perm, np.array([0, 10, 700], np.int64))


def test_segment_sums_of_ordinary_data_are_reproducible_and_within_the_fp32_bound():
    dev = util.require_gpu()
    x, _ = IR.clustered(5000, 96, 50, seed=5)
    c = IR.spherical_kmeans(x, 20, iters=3, seed=1)
    xp = _padded(x.astype(np.float32), 128)
    a, _ = KR.assign(xp, _padded(c.astype(np.float32), 128))
    a[:1200] = 3                                                # one list beyond two chunks
    order, lb = KR.lists_of(a, 20)
    xd, od, lbd = _dev(xp, dev), _i64(order, dev), _i64(lb, dev)
    got = _segment_sum(xd, od, lbd)
    again = _segment_sum(xd, od, lbd)
    assert (got.view(np.uint32) == again.view(np.uint32)).all()
    ref = KR.segment_sum(xp, order, lb)
    m = np.diff(lb)[:, None]
    bound = np.maximum(m - 1, 0) * 2.0 ** -24 * KR.segment_abs_sum(xp, order, lb)
    err = np.abs(got.astype(np.float64) - ref)
    print("max error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


# ---- k-means end to end -----------------------------------------------------------------------------------------------

def test_kmeans_end_to_end_matches_the_stand_in_run_and_is_reproducible():
    from matchmaker_amd.retrieval import spherical_kmeans
    dev = util.require_gpu()
    x, centres = IR.clustered(4000, 128, 8, seed=3, spread=0.1)
    planted = np.argmax(x.astype(np.float64) @ centres.T, axis=1)
    first = np.array([np.nonzero(planted == k)[0][0] for k in range(8)])
    init = torch.from_numpy(x[first].astype(np.float32))
    init = (init / init.norm(dim=1, keepdim=True)).to(torch.float16)
    xt = torch.from_numpy(x)
    margins, cpu_assign, gpu_assign = [], [], []

    def cpu_fn(xx, cc):
        margins.append(KR.margin_and_bound(xx.float().numpy(), cc.float().numpy())[0].min())
        out = KR.assign_fn(xx, cc)
        cpu_assign.append(out[0].numpy().copy())
        return out

    def gpu_fn(xx, cc):
        from matchmaker_amd import ops
        out = ops.kmeans_assign(xx, cc)
        gpu_assign.append(out[0].cpu().numpy())
        return out

    ref_c = spherical_kmeans(xt, 8, iters=20, init=init, assign_fn=cpu_fn, sum_fn=KR.sum_fn)
    print("smallest margin over the iterations:", min(margins))
    assert len(margins) == 20 and min(margins) >= 0.1
    xd = xt.to(dev)
    c1 = spherical_kmeans(xd, 8, iters=20, init=init.to(dev), assign_fn=gpu_fn)
    assert len(gpu_assign) == 20 and (gpu_assign[-1] == cpu_assign[-1]).all()
    final = KR.assign(x.astype(np.float32), c1.float().cpu().numpy())[0]
    assert (final == KR.assign(x.astype(np.float32), ref_c.float().numpy())[0]).all()
    c2 = spherical_kmeans(xd, 8, iters=20, init=init.to(dev))
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16))
    # and from a seeded sample
    s1, s2 = spherical_kmeans(xd, 8, iters=5, seed=4), spherical_kmeans(xd, 8, iters=5, seed=4)
    assert torch.equal(s1.view(torch.int16), s2.view(torch.int16))


# ---- the indices on the device ----------------------------------------------------------------------------------------

def _compare_search(ix, model, q, top_n):
    s, i, c = ix.search_single(q, top_n)
    rs, ri, rc = model.search_single(_padded(np.atleast_2d(q), 128), top_n)
    assert s.shape == rs.shape and s.dtype == np.float32 and i.dtype == np.int64 and c.dtype == np.int64
    assert (c == rc).all() and (i == ri).all()
    assert (s.astype(np.float64) == rs).all()                   # exact store: bit-equal, -inf padding included


def test_dynamic_index_on_the_device():
    from matchmaker_amd.retrieval import DynamicIVFIndexer
    dev = util.require_gpu()
    E, nlist, n = 96, 12, 1200
    x = KR.exact_store(n, E, seed=21)
    chunks = [x[:500], x[500:]]
    ids = [np.arange(500, dtype=np.int64) * 7 + 3, np.arange(500, n, dtype=np.int64) * 7 + 3]
    ix = DynamicIVFIndexer({"token_dim": E, "faiss_ivf_list_count": nlist}, device=dev)
    ix.prepare(chunks)
    assert ix.centroids.shape == (nlist, 128) and ix.centroids.dtype == torch.float16
    np.testing.assert_allclose(ix.centroids.float().norm(dim=1).cpu().numpy(), 1.0, atol=2e-3)
    # trained centroids rounded to multiples of 1/64: with them the centroid scores are exact in fp32 too (multiples of
    # 1/256 below 192), so the probe of every vector and query is the float64 one, ties included
    ix.centroids = (torch.round(ix.centroids.float() * 64) / 64).to(torch.float16)
    ix.index_all(ids, chunks)
    model = KR.ListModel(ix.centroids.float().cpu().numpy())
    model.add(ids[0], _padded(chunks[0], 128))
    model.add(ids[1], _padded(chunks[1], 128))
    assert ix.get_all_cluster_assignments() == [model.ids_of(l) for l in range(nlist)]
    q = KR.exact_store(17, E, seed=22)
    _compare_search(ix, model, q[0], 25)
    _compare_search(ix, model, q, 25)
    _compare_search(ix, model, q, 400)                          # beyond every list: padded
    # update of 50 ids, 10 of them unknown
    rng = np.random.default_rng(23)
    upd = np.concatenate([rng.permutation(np.concatenate(ids))[:40], np.arange(10, dtype=np.int64) * 7 + 100004])
    new = KR.exact_store(50, E, seed=24)
    ix.update(upd, new)
    model.update(upd, _padded(new, 128))
    assert ix.get_all_cluster_assignments() == [model.ids_of(l) for l in range(nlist)]
    assert ix.get_entries_from_centroids([5, 2]) == model.ids_of(5) + model.ids_of(2)
    assert ix.ids.shape[0] == n + 10
    _compare_search(ix, model, q[0], 25)
    _compare_search(ix, model, q, 25)
    # cluster_assignments of 300 queries = 300 search_single calls
    qs = KR.exact_store(300, E, seed=25)
    seq = [f"s{i}" for i in range(300)]
    got = ix.cluster_assignments(qs, seq)
    want = [[] for _ in range(nlist)]
    for i in range(300):
        want[int(ix.search_single(qs[i], 1)[2][0, 0])].append(seq[i])
    assert got == want


def test_ivf_indexer_with_native_kmeans_returns_the_exact_topk_of_the_probed_lists():
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    dev = util.require_gpu()
    n, E, nlist, nprobe, k = 6000, 128, 40, 4, 30
    x, centres = IR.clustered(n, E, nlist, seed=21, spread=1.0)
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": nprobe}
    ix = IVFFlatIPIndexer(cfg, device=dev, native_kmeans=True)
    xd = torch.from_numpy(x).to(dev)
    ix.train_resident(xd)
    c1 = ix.centroids.clone()
    ix.train_resident(xd)
    assert torch.equal(c1.view(torch.int16), ix.centroids.view(torch.int16))      # bit-equal from one seed
    ix.index_resident(torch.arange(n, device=dev) * 2 + 1, xd)
    v = ix.vectors.float().cpu().numpy().astype(np.float64)
    cent = ix.centroids.float().cpu().numpy().astype(np.float64)
    lb = ix.list_begin.cpu().numpy()
    ids = ix.ids.cpu().numpy()
    # every vector sits in the list of its best centroid, up to the accumulation noise of a near-tie
    stored = np.repeat(np.arange(nlist), np.diff(lb))
    sc = v @ cent.T
    assert lb[-1] == n and (sc[np.arange(n), stored] >= sc.max(axis=1) - 1e-3).all()
    assert (v == x.astype(np.float64)[(ids - 1) // 2]).all()
    rng = np.random.default_rng(22)
    qv = (centres[rng.integers(0, nlist, 50)] + 1.0 / np.sqrt(E) * rng.standard_normal((50, E))).astype(np.float32)
    s, i, probes = ix.search_device(qv, k, return_probes=True)
    s, i, probes = s.cpu().numpy(), i.cpu().numpy(), probes.cpu().numpy()
    q16 = qv.astype(np.float16).astype(np.float64)
    row_of = {int(e): r for r, e in enumerate(ids)}
    for r in range(50):
        union = IR.union_rows(lb, probes[r])
        full = v[union] @ q16[r]
        kk = min(k, union.size)
        got_rows = np.array([row_of[int(e)] for e in i[r, :kk]])
        assert len(set(got_rows.tolist())) == kk and np.isin(got_rows, union).all()
        got = v[got_rows] @ q16[r]
        np.testing.assert_allclose(s[r, :kk], got, atol=util.TOL_BF16, rtol=1e-3)
        rest = full[~np.isin(union, got_rows)]
        if rest.size:
            assert rest.max() <= got[kk - 1] + 1e-3 * (1 + abs(got[kk - 1])), r


def test_graph_replay_is_bit_equal_to_the_eager_calls():
    from matchmaker_amd import ops
    dev = util.require_gpu()
    x, c, a, _ = _exact_problem(1999, 128, 37)
    order, lb = KR.lists_of(a, 37)
    xd, cd, od, lbd = _dev(x, dev), _dev(c, dev), _i64(order, dev), _i64(lb, dev)
    el, es = ops.kmeans_assign(xd, cd)
    esum = ops.kmeans_segment_sum(xd, od, lbd)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ops.kmeans_assign(xd, cd)                               # warm-up on the capture stream's side
        ops.kmeans_segment_sum(xd, od, lbd)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl, gs = ops.kmeans_assign(xd, cd)
        gsum = ops.kmeans_segment_sum(xd, od, lbd)
    gl.zero_()
    gs.zero_()
    gsum.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(gl, el) and torch.equal(gs, es) and torch.equal(gsum, esum)
    assert (el.cpu().numpy() == a).all()
