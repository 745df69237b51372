"""CPU tests of the IVF inner-product index (matchmaker_amd.retrieval.IVFFlatIPIndexer, mm_ivf_scan_fwd): the C ABI, and
the indexer's host logic with the numpy restatement (tests/ivf_reference.py) standing in for the device operators."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ivf_reference as IR


def _topk_fn(q, c, k):
    s, i = IR.topk_ip(q.float().numpy(), c.float().numpy(), k)
    return torch.from_numpy(s), torch.from_numpy(i)


def _scan_fn(q, v, lb, probes, k):
    s, r = IR.ivf_scan(q.float().numpy(), v.float().numpy(), lb.numpy(), probes.numpy(), k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(r)


def _merge_fn(s, ids, k):
    s = s.clone()
    s[ids < 0] = float("-inf")
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), torch.gather(ids, 1, order)


def _indexer(E, nlist, nprobe, **kw):
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": nprobe}
    return IVFFlatIPIndexer(cfg, device="cpu", topk_fn=_topk_fn, scan_fn=_scan_fn, merge_fn=_merge_fn, **kw)


def _data(n=600, E=40, clusters=12, seed=5):
    x, _ = IR.clustered(n, E, clusters, seed)
    chunks = [x[: n // 3], x[n // 3:]]
    ids = [np.arange(0, n // 3, dtype=np.int64) * 3 + 5, np.arange(n // 3, n, dtype=np.int64) * 3 + 5]
    return x, chunks, ids


def test_header_compiles_as_c_and_the_library_exports_the_symbols(tmp_path):
    from tests import abi
    abi.run_c_client(tmp_path, r"""
#include <stdio.h>
#include <string.h>
#include "mm_native.h"
static float f[64];
static int64_t lb[4];
static int32_t pr[4];
static int64_t rows[4];
int main(void) {
  /* refused before anything touches the device */
  if (mm_ivf_scan_fwd(NULL, f, lb, pr, 8, 3, 1, 2, 128, MM_F16, 2, f, rows, f, 1u << 20, NULL) != MM_EINVAL) return 1;
  if (mm_ivf_scan_fwd(f, f, NULL, pr, 8, 3, 1, 2, 128, MM_F16, 2, f, rows, f, 1u << 20, NULL) != MM_EINVAL) return 2;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 0, 1, 2, 128, MM_F16, 2, f, rows, f, 1u << 20, NULL) != MM_EINVAL) return 3;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 3, 1, 2, 128, MM_F32, 2, f, rows, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 4;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 3, 1, 2, 100, MM_F16, 2, f, rows, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 5;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 3, 1, 2, 128, MM_F16, 4097, f, rows, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 6;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 3, 1, 4097, 128, MM_F16, 2, f, rows, f, 1u << 20, NULL) != MM_EUNSUPPORTED) return 7;
  if (mm_ivf_scan_fwd(f, f, lb, pr, 8, 3, 1, 2, 128, MM_F16, 2, f, rows, f, 16, NULL) != MM_EWORKSPACE) return 8;
  if (strlen(mm_last_error()) == 0) return 9;
  /* the candidate buffer is what a call can need at most, and never more than the larger of 2^28 and 2 n floats */
  if (mm_ivf_scan_workspace_bytes(1000, 10, 7, 3, 10) < 7000u * 4u) return 10;
  if (mm_ivf_scan_workspace_bytes(1100000, 20000, 6980, 500, 1000) > (size_t)1200 << 20) return 11;
  printf("ivf c client ok\n");
  return 0;
}
""", name="ivf_client")
    assert abi.assert_bound(("mm_ivf_scan_fwd", "mm_ivf_scan_workspace_bytes")).mm_ivf_scan_workspace_bytes(1000, 10, 7, 3, 10) > 0


def test_ops_ivf_scan_rejects_cpu_tensors_and_bad_arguments():
    from matchmaker_amd import ops, NativeError
    q, v = torch.zeros(2, 128, dtype=torch.float16), torch.zeros(8, 128, dtype=torch.float16)
    lb, pr = torch.tensor([0, 4, 8]), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(NativeError, match="CPU"):
        ops.ivf_scan(q, v, lb, pr, 2)
    m = dict(device="meta")
    qm, vm = torch.empty(2, 128, dtype=torch.float16, **m), torch.empty(8, 128, dtype=torch.float16, **m)
    lbm, prm = torch.empty(3, dtype=torch.int64, **m), torch.empty(2, 1, dtype=torch.int32, **m)
    for args in [(qm.float(), vm.float(), lbm, prm, 2), (qm, vm, lbm.int(), prm, 2), (qm, vm, lbm, prm.long(), 2),
                 (qm, vm, lbm, prm, 0), (qm, vm, lbm, prm, 4097), (qm, vm[:, :64], lbm, prm, 2),
                 (qm, vm, lbm, torch.empty(3, 1, dtype=torch.int32, **m), 2)]:
        with pytest.raises(NativeError):
            ops.ivf_scan(*args)


def test_index_layout_ids_and_search_against_the_reference():
    x, chunks, ids = _data()
    n, E, nlist = x.shape[0], x.shape[1], 16
    ix = _indexer(E, nlist, 4)
    ix.prepare(chunks)
    assert ix.centroids.shape == (nlist, 128) and ix.centroids.dtype == torch.float16
    np.testing.assert_allclose(ix.centroids.float().norm(dim=1).numpy(), 1.0, atol=2e-3)      # spherical
    ix.index(ids, chunks)
    lb = ix.list_begin.numpy()
    cent = ix.centroids.float().numpy()
    v = ix.vectors.float().numpy()
    # list ordering: every stored vector lies in the list of its best centroid, list_begin counts the assignments
    a = IR.assign(v, cent)
    assert (np.diff(a) >= 0).all() and lb[0] == 0 and lb[-1] == n
    assert (np.diff(lb) == np.bincount(a, minlength=nlist)).all()
    # id mapping: same permutation for ids and vectors, input order inside a list
    all_ids = np.concatenate(ids)
    got_ids = ix.ids.numpy()
    assert sorted(got_ids.tolist()) == sorted(all_ids.tolist())
    xp = np.zeros((n, 128), np.float32)
    xp[:, :E] = x.astype(np.float32)
    assert (v == xp[(got_ids - 5) // 3]).all()
    for l in range(nlist):
        assert (np.diff(got_ids[lb[l]: lb[l + 1]]) > 0).all()
    # search = probe selection + the exact scan of the probed lists, mapped to external ids
    qv = np.random.default_rng(1).standard_normal((7, E)).astype(np.float32)
    s, i, probes = ix.search_device(qv, 20, return_probes=True)
    assert probes.shape == (7, 4) and probes.dtype == torch.int32
    q16 = np.zeros((7, 128), np.float32)
    q16[:, :E] = qv.astype(np.float16)
    ref_p = IR.topk_ip(q16, cent, 4)[1]
    assert (probes.numpy() == ref_p).all()
    ref_s, ref_r = IR.ivf_scan(q16, v, lb, ref_p, 20)
    np.testing.assert_allclose(s.numpy(), ref_s, atol=1e-6)
    assert (i.numpy() == np.where(ref_r >= 0, got_ids[np.maximum(ref_r, 0)], -1)).all()
    s1, i1 = ix.search(qv[0], 5)                                                              # a 1-d query
    assert s1.shape == (1, 5) and (i1[0] == i.numpy()[0, :5]).all()


def test_empty_list_clamped_nprobe_and_padding():
    x, chunks, ids = _data(n=300, clusters=5)
    ix = _indexer(x.shape[1], 8, 100)                          # nprobe > nlist: clamped
    ix.prepare(chunks)
    ix.index(ids, chunks)
    # empty one list by hand: its vectors leave the index, list_begin keeps an empty range
    lb = ix.list_begin.clone()
    l = int(torch.diff(lb).argmax())
    keep = torch.ones(lb[-1].item(), dtype=torch.bool)
    keep[lb[l]: lb[l + 1]] = False
    removed = int((~keep).sum())
    ix.vectors, ix.ids = ix.vectors[keep], ix.ids[keep]
    lb[l + 1:] -= removed
    ix.list_begin = lb
    assert lb[l] == lb[l + 1]
    qv = np.random.default_rng(2).standard_normal((3, x.shape[1])).astype(np.float32)
    n_left = 300 - removed
    s, i, probes = ix.search_device(qv, n_left + 7, return_probes=True)
    assert probes.shape == (3, 8)                              # every list probed: the search is exhaustive
    assert (i[:, n_left:] == -1).all() and torch.isneginf(s[:, n_left:]).all()
    assert (i[:, :n_left] >= 0).all() and torch.isfinite(s[:, :n_left]).all()
    flat_s, flat_i = IR.topk_ip(np.pad(qv.astype(np.float16).astype(np.float32), ((0, 0), (0, 128 - x.shape[1]))),
                                ix.vectors.float().numpy(), n_left)
    np.testing.assert_allclose(s[:, :n_left].numpy(), flat_s, atol=1e-6)
    assert (i[:, :n_left].numpy() == ix.ids.numpy()[flat_i]).all()


def test_save_load_round_trip_and_probe_overwrite(tmp_path):
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    ix = _indexer(x.shape[1], 16, 3)
    ix.prepare(chunks)
    ix.index(ids, chunks)
    qv = np.random.default_rng(3).standard_normal((5, x.shape[1])).astype(np.float32)
    s0, i0 = ix.search(qv, 10)
    path = str(tmp_path / "ivf.index")
    ix.save(path)
    assert os.path.exists(path)
    ix2 = _indexer(x.shape[1], 16, 3)
    ix2.load(path)
    s1, i1 = ix2.search(qv, 10)
    assert (s0 == s1).all() and (i0 == i1).all()
    ix3 = _indexer(x.shape[1], 16, 3)
    ix3.load(path, config_overwrites={"faiss_ivf_search_probe_count": 16})
    assert ix3.nprobe == 16
    s2, i2, probes = ix3.search_device(qv, 10, return_probes=True)
    assert probes.shape == (5, 16)
    flat_s, _ = IR.topk_ip(np.pad(qv.astype(np.float16).astype(np.float32), ((0, 0), (0, 128 - x.shape[1]))),
                           ix3.vectors.float().numpy(), 10)
    np.testing.assert_allclose(s2.numpy(), flat_s, atol=1e-6)
    bogus = tmp_path / "faiss.index"
    bogus.write_bytes(b"IwFl" + bytes(64))                     # what faiss.write_index starts an IVF file with
    with pytest.raises(NativeError, match="faiss"):
        _indexer(x.shape[1], 16, 3).load(str(bogus))


def test_refuses_small_training_sets_fp32_and_subsamples_reproducibly():
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    x, chunks, ids = _data(n=60)
    with pytest.raises(NativeError, match="training vectors"):
        _indexer(x.shape[1], 64, 4).prepare(chunks)
    with pytest.raises(NativeError, match="float16"):
        IVFFlatIPIndexer({"token_dim": 40, "token_dtype": "float32", "faiss_ivf_list_count": 4,
                          "faiss_ivf_search_probe_count": 2}, device="cpu")
    a, b = _indexer(x.shape[1], 4, 2), _indexer(x.shape[1], 4, 2)
    a.prepare(chunks, subsample=0.5)
    b.prepare(chunks, subsample=0.5)
    assert torch.equal(a.centroids, b.centroids)              # a fixed seed gives a reproducible index


# ---- the two exact problems of the GPU suite: the restatement against a plain sort ---------------------------------------

def _sorted_topk(q, v, lb, probes, k):
    """(score descending, row ascending) by one lexsort per query; nothing of ivf_reference.ivf_scan is used"""
    out_s, out_r = np.full((q.shape[0], k), -np.inf), np.full((q.shape[0], k), -1, np.int64)
    for i in range(q.shape[0]):
        rows = np.array(sorted(r for l in probes[i] if l >= 0 for r in range(lb[l], lb[l + 1])), np.int64)
        s = v[rows].astype(np.float64) @ q[i].astype(np.float64)
        order = np.lexsort((rows, -s))[:k]
        out_s[i, : order.size], out_r[i, : order.size] = s[order], rows[order]
    return out_s, out_r


def test_carry_problem_reaches_past_the_tile_and_the_restatement_equals_a_plain_sort():
    q, v, lb, probes, k = IR.carry_problem()
    lens = np.diff(lb)
    assert lens.size == 1030 and q.shape == (1030, 128) and lb[-1] == v.shape[0] == 2000 and probes.shape == (1030, 3) and k == 5
    assert (lens == 0).sum() >= 5 and np.median(lens) in (1, 2)
    for i in range(1024, 1030):                                  # queries behind the tile probe non-empty lists behind the tile
        assert any(l >= 1024 and lens[l] > 0 for l in probes[i]), i
    assert all(len(set(p.tolist())) == 3 for p in probes)
    assert np.abs(v).max() <= 2 and np.abs(q).max() <= 2         # |score| <= 512: exact in fp16 inputs and any fp32 order
    ref_s, ref_r = IR.ivf_scan(q, v, lb, probes, k)
    srt_s, srt_r = _sorted_topk(q, v, lb, probes, k)
    assert np.array_equal(ref_r, srt_r) and np.array_equal(ref_s, srt_s)
    assert (ref_r[:, -1] == -1).any() and (ref_r[:, -1] >= 0).any()      # unions shorter and longer than k


def test_tie_problem_has_40_ties_from_rank_8_and_the_restatement_equals_a_plain_sort():
    q, v, lb, probes, k, group = IR.tie_problem()
    assert k == 10 and group.size == 40 and (v[group] == v[group[0]]).all()
    in_list = [int(((group >= lb[l]) & (group < lb[l + 1])).sum()) for l in range(lb.size - 1)]
    assert in_list == [0, 20, 0, 0, 20] and set(probes[0].tolist()) == {4, -1, 1}
    ref_s, ref_r = IR.ivf_scan(q, v, lb, probes, k)
    srt_s, srt_r = _sorted_topk(q, v, lb, probes, k)
    assert np.array_equal(ref_r, srt_r) and np.array_equal(ref_s, srt_s)
    assert ref_s[0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0, 0, 0] and ref_r[0, 7:].tolist() == group[:3].tolist()
    full = v[np.concatenate([np.arange(lb[1], lb[2]), np.arange(lb[4], lb[5])])] @ q[0]
    assert (full == 0).sum() == 40 and (full > 0).sum() == 7     # nothing else ties with the group


# ---- sharded IVF index under gloo ---------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ivf_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from matchmaker_amd.sharding import shard_range
    x, chunks, ids = _data(n=601)                               # odd size: uneven shards
    ix = _indexer(x.shape[1], 16, 5)
    ix.prepare(chunks)
    ix.index(ids, chunks)
    lo, hi = shard_range(601, world, rank)
    assert ix.vectors.shape == (hi - lo, 128) and sorted(ix.ids.tolist()) == np.concatenate(ids)[lo:hi].tolist()
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    ix.save(os.path.join(out_dir, "ivf.index"))
    np.save(os.path.join(out_dir, f"cent{rank}.npy"), ix.centroids.numpy())
    np.save(os.path.join(out_dir, f"s{rank}.npy"), s)
    np.save(os.path.join(out_dir, f"i{rank}.npy"), i)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_sharded_ivf_equals_single_process(tmp_path):
    world = 2
    mp.spawn(_ivf_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    c0, c1 = np.load(tmp_path / "cent0.npy"), np.load(tmp_path / "cent1.npy")
    assert (c0 == c1).all()                                     # both ranks probe the same lists
    assert (np.load(tmp_path / "i0.npy") == np.load(tmp_path / "i1.npy")).all()
    assert os.path.exists(tmp_path / "ivf.index.rank0") and os.path.exists(tmp_path / "ivf.index.rank1")
    x, chunks, ids = _data(n=601)
    ix = _indexer(x.shape[1], 16, 5)
    ix.prepare(chunks)
    assert (ix.centroids.numpy() == c0).all()
    ix.index(ids, chunks)
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    np.testing.assert_allclose(np.load(tmp_path / "s0.npy"), s, atol=1e-6)
    # same probed lists, same vectors: the merged result is the single-process result wherever scores are distinct
    distinct = np.ones_like(s, bool)
    distinct[:, 1:] &= np.diff(s, axis=1) != 0
    distinct[:, :-1] &= np.diff(s, axis=1) != 0
    assert (np.load(tmp_path / "i0.npy")[distinct] == i[distinct]).all()


def test_reference_assignment_has_few_near_ties_on_the_gpu_suite_collection():
    """tests/test_ivf_gpu.py caps the vectors stored in a near-tie list at 1 %: on its collection and seed the reference
    alone must stay far under that cap (vectors whose two best centroids are within the tolerance)."""
    x, _ = IR.clustered(30000, 128, 200, 21, spread=1.0)
    cent = IR.spherical_kmeans(x, 200, iters=20, seed=0)
    sc = np.sort(x.astype(np.float64) @ cent.astype(np.float64).T, axis=1)
    near = int((sc[:, -1] - sc[:, -2] <= 1e-3 * (1 + np.abs(sc[:, -1]))).sum())
    assert near < 0.005 * x.shape[0], near
