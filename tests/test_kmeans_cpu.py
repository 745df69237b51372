"""CPU tests of the k-means operators and the dynamic IVF index (mm_kmeans_assign, mm_kmeans_segment_sum,
matchmaker_amd.retrieval.spherical_kmeans / DynamicIVFIndexer): the C ABI, and the host logic with the numpy restatement
(tests/kmeans_reference.py) standing in for the device operators."""
import os

import numpy as np
import pytest
import torch

from tests import ivf_reference as IR
from tests import kmeans_reference as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm_kmeans_assign", "mm_kmeans_segment_sum_workspace_bytes", "mm_kmeans_segment_sum")


def _dyn(E, nlist, **cfg):
    from matchmaker_amd.retrieval import DynamicIVFIndexer
    cfg = dict({"token_dim": E, "faiss_ivf_list_count": nlist}, **cfg)
    return DynamicIVFIndexer(cfg, device="cpu", assign_fn=KR.assign_fn, sum_fn=KR.sum_fn, scan_fn=KR.scan_fn)


def _data(n=600, E=40, clusters=12, seed=5):
    x, _ = IR.clustered(n, E, clusters, seed)
    chunks = [x[: n // 3], x[n // 3:]]
    ids = [np.arange(0, n // 3, dtype=np.int64) * 3 + 5, np.arange(n // 3, n, dtype=np.int64) * 3 + 5]
    return x, chunks, ids


def _pad(a, E_pad=128):
    out = np.zeros((a.shape[0], E_pad), np.float32)
    out[:, : a.shape[1]] = a.astype(np.float16)
    return out


def test_symbols_are_declared_bound_and_the_abi_version_stays_4():
    from matchmaker_amd import _lib
    from tests import abi
    L = abi.assert_bound(SYMBOLS)
    header = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    for cite in ("faiss_indices.py:323-352, 401-428", "query_clusterer.py:218-221"):
        assert cite in header
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    assert L.mm_kmeans_segment_sum_workspace_bytes(5000, 3, 128) >= (5000 // 512) * 128 * 4


def test_c_client_is_refused_before_anything_touches_the_device(tmp_path):
    from tests import abi
    abi.run_c_client(tmp_path, r"""
#include <stdio.h>
#include <string.h>
#include "mm_native.h"
static float f[64];
static int32_t li[4];
static int64_t lb[4], order[4];
int main(void) {
  if (mm_kmeans_assign(NULL, f, 4, 3, 128, MM_F16, li, f, NULL) != MM_EINVAL) return 1;
  if (mm_kmeans_assign(f, NULL, 4, 3, 128, MM_F16, li, f, NULL) != MM_EINVAL) return 2;
  if (mm_kmeans_assign(f, f, 4, 3, 128, MM_F16, NULL, f, NULL) != MM_EINVAL) return 3;
  if (mm_kmeans_assign(f, f, 4, 3, 128, MM_F16, li, NULL, NULL) != MM_EINVAL) return 4;
  if (mm_kmeans_assign(f, f, 4, 0, 128, MM_F16, li, f, NULL) != MM_EUNSUPPORTED) return 5;
  if (mm_kmeans_assign(f, f, 4, 65537, 128, MM_F16, li, f, NULL) != MM_EUNSUPPORTED) return 6;
  if (mm_kmeans_assign(f, f, 4, 3, 100, MM_F16, li, f, NULL) != MM_EUNSUPPORTED) return 7;
  if (mm_kmeans_assign(f, f, 4, 3, 128, MM_F32, li, f, NULL) != MM_EUNSUPPORTED) return 8;
  if (mm_kmeans_assign(f, f, (int64_t)1 << 31, 3, 128, MM_F16, li, f, NULL) != MM_EUNSUPPORTED) return 9;
  /* no rows: success, and nothing is launched (no device exists here) */
  if (mm_kmeans_assign(NULL, f, 0, 3, 128, MM_F16, li, f, NULL) != MM_OK) return 10;
  if (mm_kmeans_segment_sum(NULL, order, lb, 4, 3, 128, MM_F16, f, f, 1u << 20, NULL) != MM_EINVAL) return 11;
  if (mm_kmeans_segment_sum(f, NULL, lb, 4, 3, 128, MM_F16, f, f, 1u << 20, NULL) != MM_EINVAL) return 12;
  if (mm_kmeans_segment_sum(f, order, NULL, 4, 3, 128, MM_F16, f, f, 1u << 20, NULL) != MM_EINVAL) return 13;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 3, 128, MM_F16, NULL, f, 1u << 20, NULL) != MM_EINVAL) return 14;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 0, 128, MM_F16, f, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 15;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 65537, 128, MM_F16, f, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 16;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 3, 100, MM_F16, f, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 17;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 3, 128, MM_F32, f, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 18;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 3, 128, MM_F16, f, f, 16, NULL) != MM_EWORKSPACE) return 19;
  if (mm_kmeans_segment_sum(f, order, lb, 4, 3, 128, MM_F16, f, NULL, 1u << 20, NULL) != MM_EWORKSPACE) return 20;
  if (strlen(mm_last_error()) == 0) return 21;
  /* the chunk partials of the longest possible split, and the task table */
  if (mm_kmeans_segment_sum_workspace_bytes(5000, 1, 128) < (5000u / 512u + 1u) * 128u * 4u + 8u) return 22;
  if (mm_kmeans_segment_sum_workspace_bytes(1100000, 2500, 768) > (size_t)32 << 20) return 23;
  printf("kmeans c client ok\n");
  return 0;
}
""", name="kmeans_client")


def test_ops_refuse_cpu_tensors_mixed_dtypes_and_wrong_shapes():
    from matchmaker_amd import ops, NativeError
    x, c = torch.zeros(8, 128, dtype=torch.float16), torch.zeros(3, 128, dtype=torch.float16)
    order, lb = torch.arange(8), torch.tensor([0, 4, 8, 8])
    with pytest.raises(NativeError, match="CPU"):
        ops.kmeans_assign(x, c)
    with pytest.raises(NativeError, match="CPU"):
        ops.kmeans_segment_sum(x, order, lb)
    m = dict(device="meta")
    xm, cm = torch.empty(8, 128, dtype=torch.float16, **m), torch.empty(3, 128, dtype=torch.float16, **m)
    om, lbm = torch.empty(8, dtype=torch.int64, **m), torch.empty(4, dtype=torch.int64, **m)
    for args in [(xm, cm.bfloat16()), (xm.float(), cm.float()), (xm, cm[:, :64]), (xm[0], cm), (xm, cm[0]),
                 (xm, torch.empty(0, 128, dtype=torch.float16, **m)), (xm, torch.empty(65537, 128, dtype=torch.float16, **m)),
                 (torch.empty(8, 96, dtype=torch.float16, **m), torch.empty(3, 96, dtype=torch.float16, **m))]:
        with pytest.raises(NativeError):
            ops.kmeans_assign(*args)
    for args in [(xm.float(), om, lbm), (xm, om.int(), lbm), (xm, om, lbm.int()), (xm, om[:7], lbm), (xm, om, lbm[:1]),
                 (xm[0], om, lbm), (xm, om[:, None], lbm), (torch.empty(8, 96, dtype=torch.float16, **m), om, lbm),
                 (xm, om, torch.empty(65538, dtype=torch.int64, **m))]:
        with pytest.raises(NativeError):
            ops.kmeans_segment_sum(*args)


def test_spherical_kmeans_with_stand_ins_follows_the_reference_loop():
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import spherical_kmeans
    x, _ = IR.clustered(500, 40, 9, seed=2)
    xt = torch.from_numpy(x)
    init = torch.from_numpy(_pad(x[:9] / np.linalg.norm(x[:9].astype(np.float64), axis=1, keepdims=True)))
    cent = spherical_kmeans(xt, 9, iters=4, init=init, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)
    assert cent.shape == (9, 128) and cent.dtype == torch.float16
    np.testing.assert_allclose(cent.float().norm(dim=1).numpy(), 1.0, atol=2e-3)
    # the same loop in float64 numpy from the same start: identical assignments at the end
    c = init.to(torch.float16).float().numpy()
    xp = _pad(x)
    for _ in range(4):
        a, _s = KR.assign(xp, c)
        order, lb = KR.lists_of(a, 9)
        assert (np.diff(lb) > 0).all()
        sums = KR.segment_sum(xp, order, lb)
        c = (sums / np.linalg.norm(sums, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
    assert (KR.assign(xp, cent.float().numpy())[0] == KR.assign(xp, c)[0]).all()
    # a seeded start is reproducible, another seed gives another sample
    a = spherical_kmeans(xt, 9, iters=2, seed=7, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)
    b = spherical_kmeans(xt, 9, iters=2, seed=7, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)
    assert torch.equal(a, b)
    assert not torch.equal(a, spherical_kmeans(xt, 9, iters=2, seed=8, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn))
    # an empty cluster is re-seeded from the largest one: two identical starts leave the higher-numbered one empty
    init2 = init.clone()
    init2[8] = init2[0]
    c2 = spherical_kmeans(xt, 9, iters=1, init=init2, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)
    a0 = KR.assign(xp, init2.to(torch.float16).float().numpy())[0]
    assert (a0 != 8).all()
    big = np.bincount(a0, minlength=9).argmax()
    first = xp[np.nonzero(a0 == big)[0][0]]
    np.testing.assert_allclose(c2[8].float().numpy(), first / np.linalg.norm(first), atol=1e-3)
    with pytest.raises(NativeError, match="training vectors"):
        spherical_kmeans(xt[:5], 9, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)
    with pytest.raises(NativeError, match="init"):
        spherical_kmeans(xt, 9, init=init[:8], assign_fn=KR.assign_fn, sum_fn=KR.sum_fn)


def test_prepare_selects_the_rows_of_the_reference_and_refuses_one_chunk():
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import DynamicIVFIndexer
    rng = np.random.default_rng(0)
    chunks = [rng.standard_normal((n, 24)).astype(np.float32) for n in (200, 150, 90)]
    total, sub = 440, 0.3
    # faiss_indices.py:335-345 restated: RandomState(123), one choice per chunk but the last, in chunk order
    per = int(total * sub) // (len(chunks) - 1)
    rs = np.random.RandomState(123)
    want = [rs.choice(c.shape[0], size=per, replace=False) for c in chunks[:-1]]
    got = DynamicIVFIndexer.train_rows([c.shape[0] for c in chunks], sub)
    assert len(got) == 2 and all((g == w).all() for g, w in zip(got, want)) and per == 66
    seen = []

    def spy(x, c):
        seen.append(x.float().numpy().copy())
        return KR.assign_fn(x, c)

    ix = DynamicIVFIndexer({"token_dim": 24, "faiss_ivf_list_count": 5}, device="cpu", assign_fn=spy, sum_fn=KR.sum_fn,
                           scan_fn=KR.scan_fn)
    ix.prepare(chunks, subsample=sub)
    # trained on exactly those rows (no zero rows appended), in that order
    rows = np.concatenate([c[w] for c, w in zip(chunks, want)])
    assert seen[0].shape == (2 * per, 128) and (seen[0][:, :24] == rows.astype(np.float16).astype(np.float32)).all()
    assert ix.centroids.shape == (5, 128)
    ix.prepare(chunks)                                          # -1: everything
    assert seen[DynamicIVFIndexer.KMEANS_ITERS].shape == (total, 128)
    with pytest.raises(NativeError, match="two chunks"):
        ix.prepare(chunks[:1], subsample=0.5)
    with pytest.raises(NativeError, match="training vectors"):
        _dyn(24, 500).prepare(chunks)
    with pytest.raises(NativeError, match="float16"):
        DynamicIVFIndexer({"token_dim": 24, "faiss_ivf_list_count": 5, "token_dtype": "float32"}, device="cpu")
    with pytest.raises(NativeError, match="prepare"):
        _dyn(24, 5).index_all([np.arange(3)], [chunks[0]])


def _check_against_model(ix, model, qv, top_n):
    vec, ids, lb = model.layout()
    assert (ix.list_begin.numpy() == lb).all() and (ix.ids.numpy() == ids).all()
    assert (ix.vectors.float().numpy() == vec).all()
    assert ix.get_all_cluster_assignments() == [model.ids_of(l) for l in range(len(model.lists))]
    assert ix.get_entries_from_centroids([3, 0, 3]) == model.ids_of(3) + model.ids_of(0) + model.ids_of(3)
    s, i, c = ix.search_single(qv, top_n)
    rs, ri, rc = model.search_single(_pad(qv), top_n)
    assert s.dtype == np.float32 and i.dtype == np.int64 and c.dtype == np.int64 and c.shape == (qv.shape[0], 1)
    assert (c == rc).all() and (i == ri).all()
    np.testing.assert_allclose(s, rs, atol=1e-6)
    return i


def test_index_all_update_entries_and_search_single():
    x, chunks, ids = _data()
    E = x.shape[1]
    ix = _dyn(E, 8)
    ix.prepare(chunks)
    # index_all truncates every chunk to len(ids[i]) (faiss_indices.py:359)
    short = [ids[0][:150], ids[1]]
    ix.index_all(short, chunks)
    model = KR.ListModel(ix.centroids.float().numpy())
    model.add(short[0], _pad(chunks[0][:150]))
    model.add(short[1], _pad(chunks[1]))
    assert ix.ids.shape[0] == 550 and ix.list_n_probe == 1 and ix.faiss_ivf_list_count == 8
    qv = np.random.default_rng(1).standard_normal((6, E)).astype(np.float32)
    i = _check_against_model(ix, model, qv, 12)
    assert (i >= 0).any()
    s1, i1, c1 = ix.search_single(qv[0], 4)                     # a 1-d query
    assert s1.shape == (1, 4) and c1.shape == (1, 1) and (i1[0] == i[0, :4]).all()
    # top_n beyond the list: (-inf, -1) padding
    s, ii, _ = ix.search_single(qv[:2], 600)
    assert (ii[:, -1] == -1).all() and np.isneginf(s[:, -1]).all()
    # update: 40 known ids get new vectors (they leave their lists and arrive at the end of the new ones), 10 unknown ids
    # are simply added; one more row of data than ids is ignored
    rng = np.random.default_rng(3)
    known = rng.permutation(np.concatenate(short))[:40]
    upd_ids = np.concatenate([known, np.arange(10, dtype=np.int64) * 3 + 4000])
    new, _ = IR.clustered(51, E, 12, seed=9)
    before = ix.get_all_cluster_assignments()
    ix.update(list(upd_ids), new)
    model.update(upd_ids, _pad(new))
    _check_against_model(ix, model, qv, 12)
    after = ix.get_all_cluster_assignments()
    assert sorted(sum(after, [])) == sorted(set(np.concatenate(short).tolist()) | set(upd_ids.tolist()))
    gone = set(upd_ids.tolist())
    for l in range(8):
        kept = [e for e in before[l] if e not in gone]
        assert after[l][: len(kept)] == kept                    # untouched entries keep their order, ahead of the arrivals
        assert set(after[l][len(kept):]) <= gone
    assert (ix.centroids.float().numpy() == model.centroids).all()      # the centroids do not move


def test_cluster_assignments_equal_a_per_query_loop():
    x, chunks, ids = _data()
    E = x.shape[1]
    ix = _dyn(E, 8)
    ix.prepare(chunks)
    ix.index_all(ids, chunks)
    qv = np.random.default_rng(2).standard_normal((40, E)).astype(np.float32)
    seq_ids = [f"q{i}" for i in range(40)]
    got = ix.cluster_assignments(qv, seq_ids)
    want = [[] for _ in range(8)]
    for i, sid in enumerate(seq_ids):                           # query_clusterer.py:218-221
        _, _, c = ix.search_single(qv[i], 1)
        want[int(c[0, 0])].append(sid)
    assert got == want and sum(len(c) for c in got) == 40
    a = ix.assign(qv)
    assert a.dtype == torch.int64 and a.shape == (40,)
    assert (a.numpy() == KR.assign(_pad(qv), ix.centroids.float().numpy())[0]).all()


def test_ivf_indexer_native_kmeans_gives_the_centroids_of_the_default_path():
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    from tests.test_ivf_cpu import _topk_fn, _scan_fn, _merge_fn
    x, chunks, ids = _data()
    cfg = {"token_dim": x.shape[1], "faiss_ivf_list_count": 16, "faiss_ivf_search_probe_count": 4}
    kw = dict(device="cpu", topk_fn=_topk_fn, scan_fn=_scan_fn, merge_fn=_merge_fn)
    old = IVFFlatIPIndexer(cfg, **kw)
    new = IVFFlatIPIndexer(cfg, native_kmeans=True, assign_fn=KR.assign_fn, sum_fn=KR.sum_fn, **kw)
    assert old.native_kmeans is False
    for sub in (-1, 0.5):
        old.prepare(chunks, subsample=sub)
        new.prepare(chunks, subsample=sub)
        assert torch.equal(old.centroids, new.centroids)
    old.index(ids, chunks)
    new.index(ids, chunks)
    assert torch.equal(old.list_begin, new.list_begin) and torch.equal(old.ids, new.ids) and torch.equal(old.vectors, new.vectors)
    qv = np.random.default_rng(1).standard_normal((5, x.shape[1])).astype(np.float32)
    (s0, i0), (s1, i1) = old.search(qv, 10), new.search(qv, 10)
    assert (s0 == s1).all() and (i0 == i1).all()


def test_package_exports_the_indexers():
    import matchmaker_amd
    from matchmaker_amd import retrieval
    assert matchmaker_amd.DynamicIVFIndexer is retrieval.DynamicIVFIndexer
    assert matchmaker_amd.IVFFlatIPIndexer is retrieval.IVFFlatIPIndexer
