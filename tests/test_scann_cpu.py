"""CPU tests of the quantized index (matchmaker_amd.retrieval.ScannIPIndexer; mm_ah_encode, mm_ah_scan_fwd, mm_gather_dot):
the C ABI and its binding, the argument checks, the nibble layout, the restatement's own agreement between float32 and
float64 on the inputs tests/test_scann_gpu.py uses, and the indexer's host logic with the numpy restatement
(tests/scann_reference.py) standing in for the device operators."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ivf_reference as IR
from tests import scann_reference as SR

SYMBOLS = ("mm_ah_encode", "mm_ah_scan_workspace_bytes", "mm_ah_scan_fwd", "mm_gather_dot")


def _indexer(E, **cfg):
    from matchmaker_amd.retrieval import ScannIPIndexer
    c = {"token_dim": E, "token_dtype": "float16", "query_sets": {"dev": {"top_n": 30}}}
    c.update(cfg)
    return ScannIPIndexer(c, device="cpu", topk_fn=SR.topk_fn, encode_fn=SR.encode_fn, scan_fn=SR.scan_fn,
                          rescore_fn=SR.rescore_fn, merge_fn=SR.merge_fn)


def _data(n=600, E=40, clusters=12, seed=5):
    x, _ = IR.clustered(n, E, clusters, seed)
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
    assert "ah_scan.hip" in build.SOURCES and "ah_encode.hip" in build.SOURCES
    assert any(h.endswith("ivf_device.h") for h in build.HEADERS)          # the shared scan scaffolding triggers rebuilds
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    # the scan's workspace is the IVF scan's
    assert L.mm_ah_scan_workspace_bytes(1000, 10, 7, 3, 10) == L.mm_ivf_scan_workspace_bytes(1000, 10, 7, 3, 10) > 7000 * 4
    assert L.mm_ah_scan_workspace_bytes(1000, 0, 7, 3, 10) == 0


def test_arguments_are_refused_before_any_launch():
    from matchmaker_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(1 << 12, dtype=torch.float32).data_ptr()
    F16, F32 = _lib.MM_F16, _lib.MM_F32

    def scan(q=buf, codes=buf, n=8, nlist=3, nq=1, nprobe=2, E=128, dt=F16, k=2, ws=buf, wsb=1 << 20):
        return L.mm_ah_scan_fwd(q, codes, buf, buf, buf, buf, n, nlist, nq, nprobe, E, dt, k, buf, buf, ws, wsb, None)

    assert scan(q=None) == _lib.MM_EINVAL and scan(nlist=0) == _lib.MM_EINVAL and scan(k=0) == _lib.MM_EINVAL
    assert scan(q=buf + 4) == _lib.MM_EINVAL                                   # alignment
    for bad in (dict(dt=F32), dict(E=100), dict(E=896), dict(k=4097), dict(nprobe=4097), dict(n=1 << 31)):
        assert scan(**bad) == _lib.MM_EUNSUPPORTED, bad
    assert scan(wsb=16) == _lib.MM_EWORKSPACE and scan(ws=None) == _lib.MM_EWORKSPACE
    assert L.mm_last_error()

    def enc(x=buf, n=4, nlist=2, E=128, dt=F16, eta=2.0, passes=1):
        return L.mm_ah_encode(x, buf, buf, buf, n, nlist, E, dt, eta, passes, buf, None)

    assert enc(n=0) == _lib.MM_OK                                              # nothing to do: no launch
    assert enc(x=None) == _lib.MM_EINVAL and enc(nlist=0) == _lib.MM_EINVAL and enc(n=-1) == _lib.MM_EINVAL
    for bad in (dict(dt=F32), dict(E=64), dict(eta=-1.0), dict(eta=float("nan")), dict(eta=float("inf")), dict(passes=-1),
                dict(passes=65)):
        assert enc(**bad) == _lib.MM_EUNSUPPORTED, bad

    def gd(q=buf, n=4, nq=1, R=3, E=128, dt=F16):
        return L.mm_gather_dot(q, buf, buf, n, nq, R, E, dt, buf, None)

    assert gd(q=None) == _lib.MM_EINVAL and gd(R=0) == _lib.MM_EINVAL and gd(nq=0) == _lib.MM_EINVAL and gd(q=buf + 2) == _lib.MM_EINVAL
    assert gd(dt=F32) == _lib.MM_EUNSUPPORTED and gd(E=96) == _lib.MM_EUNSUPPORTED


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from matchmaker_amd import ops, NativeError
    h = torch.float16
    with pytest.raises(NativeError, match="CPU"):
        ops.ah_scan(torch.zeros(2, 128, dtype=h), torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(64, 16, 2, dtype=h),
                    torch.tensor([0, 4, 8]), torch.zeros(2, 1, dtype=torch.int32), torch.zeros(2, 1), 2)
    with pytest.raises(NativeError, match="CPU"):
        ops.gather_dot(torch.zeros(2, 128, dtype=h), torch.zeros(8, 128, dtype=h), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(NativeError, match="CPU"):
        ops.ah_encode(torch.zeros(2, 128, dtype=h), torch.zeros(2, dtype=torch.int32), torch.zeros(3, 128, dtype=h),
                      torch.zeros(64, 16, 2, dtype=h), 2.0)
    m = dict(device="meta")
    q, codes, cb = torch.empty(2, 128, dtype=h, **m), torch.empty(8, 32, dtype=torch.uint8, **m), torch.empty(64, 16, 2, dtype=h, **m)
    lb, pr, ps = torch.empty(3, dtype=torch.int64, **m), torch.empty(2, 1, dtype=torch.int32, **m), torch.empty(2, 1, **m)
    for args in [(q.float(), codes, cb.float(), lb, pr, ps, 2), (q, codes.int(), cb, lb, pr, ps, 2), (q, codes[:, :16], cb, lb, pr, ps, 2),
                 (q, codes, cb[:32], lb, pr, ps, 2), (q, codes, cb.bfloat16(), lb, pr, ps, 2), (q, codes, cb, lb.int(), pr, ps, 2),
                 (q, codes, cb, lb, pr.long(), ps, 2), (q, codes, cb, lb, pr, ps.double(), 2),
                 (q, codes, cb, lb, pr, torch.empty(2, 2, **m), 2), (q, codes, cb, lb, pr, ps, 0), (q, codes, cb, lb, pr, ps, 4097),
                 (q, codes, cb, lb, torch.empty(3, 1, dtype=torch.int32, **m), ps, 2)]:
        with pytest.raises(NativeError):
            ops.ah_scan(*args)
    v, rows = torch.empty(8, 128, dtype=h, **m), torch.empty(2, 3, dtype=torch.int64, **m)
    for args in [(q.float(), v.float(), rows), (q, v[:, :64], rows), (q, v, rows.int()), (q, v, rows[:1]), (q, v.bfloat16(), rows)]:
        with pytest.raises(NativeError):
            ops.gather_dot(*args)
    x, li, ce = torch.empty(5, 128, dtype=h, **m), torch.empty(5, dtype=torch.int32, **m), torch.empty(3, 128, dtype=h, **m)
    for args in [(x.float(), li, ce.float(), cb.float(), 2.0), (x, li.long(), ce, cb, 2.0), (x, li[:4], ce, cb, 2.0),
                 (x, li, ce[:, :64], cb, 2.0), (x, li, ce, cb[:, :8], 2.0), (x, li, ce, cb, -1.0), (x, li, ce, cb, float("nan")),
                 (x, li, ce, cb, 2.0, 65), (x[:, :96], li, ce[:, :96], cb[:48], 2.0)]:
        with pytest.raises(NativeError):
            ops.ah_encode(*args)


def test_nibble_layout_and_decode():
    blocks = np.array([[1, 2, 3, 15], [0, 9, 14, 4]], np.uint8)
    codes = SR.pack(blocks)
    assert codes.tolist() == [[0x21, 0xF3], [0x90, 0x4E]]                      # the even block in the low nibble
    assert (SR.unpack(codes) == blocks).all()
    cb = np.arange(4 * 16 * 2, dtype=np.float32).reshape(4, 16, 2)
    assert SR.decode(codes, cb)[0].tolist() == [2, 3, 36, 37, 70, 71, 126, 127]


def test_encoder_restatement_on_a_hand_checked_block_and_plain_quantisation():
    x, lists, cent, cb = SR.exact_store(40, 128, 5, seed=1)
    pq = SR.encode(x, lists, cent, cb, 1.0, 2)
    r = (x - cent[lists]).reshape(40, 64, 2)
    near = np.argmin(((r[:, :, None, :] - cb[None]) ** 2).sum(-1), axis=2)
    assert (SR.unpack(pq) == near).all()                                       # eta = 1: the nearest codeword
    assert (SR.encode(x, lists, cent, cb, 31.96, 0) == pq).all()              # passes = 0: the same
    eta = 127 * 0.04 / 0.96
    c2 = SR.encode(x, lists, cent, cb, eta, 2)
    l0, l2 = SR.loss(x, lists, cent, cb, pq, eta), SR.loss(x, lists, cent, cb, c2, eta)
    assert (l2 <= l0 * (1 + 1e-9)).all() and (l2 < l0).any()                   # the descent never loses, and moves something


def test_float32_and_float64_restatements_agree_on_the_gpu_suite_inputs():
    """tests/test_scann_gpu.py compares the kernel's codes with the float32 restatement: bit for bit on the exact-arithmetic
    store, and up to blocks whose two best costs nearly tie on random data (capped at 1 % of the blocks).  The restatement
    alone must agree with its float64 twin on every code of the first input, and stay under the cap on the second."""
    from tests import test_scann_gpu as G
    for E in (128, 768):
        x, lists, cent, cb = SR.exact_store(G.EXACT_N, E, G.EXACT_NLIST, seed=G.EXACT_SEED)
        x, lists, cent = G.plant_exact_rows(x, lists, cent, cb)
        for eta, passes in ((1.0, 2), (G.eta_of(E), 1), (G.eta_of(E), 2)):
            a = SR.encode(x, lists, cent, cb, eta, passes)
            b = SR.encode(x, lists, cent, cb, eta, passes, dtype=np.float64)
            assert (a == b).all(), (E, eta, passes)
    for E in (128, 768):
        x, lists, cent, cb = G.random_encode_problem(1000, E)
        a = SR.unpack(SR.encode(x, lists, cent, cb, G.eta_of(E), 2))
        b = SR.unpack(SR.encode(x, lists, cent, cb, G.eta_of(E), 2, dtype=np.float64))
        differ = int((a != b).sum())
        print(f"E {E}: float32 and float64 restatements differ on {differ} of {a.size} blocks")
        assert differ < 0.01 * a.size


def test_defaults_come_from_the_config():
    from matchmaker_amd import NativeError, ScannIPIndexer
    ix = _indexer(40)
    assert (ix.leaves_to_search, ix.reorder, ix.threshold, ix.num_leaves) == (100, 30, 0.2, None)
    assert abs(ix.eta - 39 * 0.04 / 0.96) < 1e-12                              # (token_dim - 1) T^2 / (1 - T^2)
    ix = _indexer(40, query_sets={"a": {"top_n": 30, "index_hit_top_n": 77}, "b": {"top_n": 5}})
    assert ix.reorder == 77                                                    # the FIRST query set, index_hit_top_n first
    ix = _indexer(40, scann_num_leaves=9, scann_leaves_to_search=4, scann_reorder=11, scann_anisotropic_threshold=0.5)
    assert (ix.num_leaves, ix.leaves_to_search, ix.reorder) == (9, 4, 11) and abs(ix.eta - 39 * 0.25 / 0.75) < 1e-12
    with pytest.raises(NativeError, match="float16"):
        ScannIPIndexer({"token_dim": 40, "token_dtype": "float32", "query_sets": {"d": {"top_n": 3}}}, device="cpu")
    with pytest.raises(NativeError, match="query_sets"):
        ScannIPIndexer({"token_dim": 40, "token_dtype": "float16"}, device="cpu")
    for bad in (dict(scann_num_leaves=0), dict(scann_leaves_to_search=0), dict(scann_reorder=0), dict(scann_anisotropic_threshold=1.0)):
        with pytest.raises(NativeError):
            _indexer(40, **bad)
    with pytest.raises(NativeError, match="index"):
        _indexer(40).search(np.zeros(40, np.float32), 3)
    assert _indexer(40).prepare([np.zeros((3, 40))]) is None                   # a no-op


def test_index_layout_codes_and_search_against_the_restatement():
    x, chunks, ids = _data()
    n, E = x.shape
    ix = _indexer(E, scann_leaves_to_search=5)
    ix.index(ids, chunks)
    assert ix.nlist == int(np.sqrt(n)) == 24 and ix.centroids.shape == (24, 128) and ix.codebook.shape == (64, 16, 2)
    assert ix.codes.shape == (n, 32) and ix.codes.dtype == torch.uint8 and ix.vectors.shape == (n, 128)
    lb, cent, v = ix.list_begin.numpy(), ix.centroids.float().numpy(), ix.vectors.float().numpy()
    a = IR.assign(v, cent)
    assert (np.diff(a) >= 0).all() and lb[0] == 0 and lb[-1] == n and (np.diff(lb) == np.bincount(a, minlength=24)).all()
    got_ids = ix.ids.numpy()
    assert sorted(got_ids.tolist()) == np.concatenate(ids).tolist()
    assert (v == _padded16(x)[(got_ids - 5) // 3]).all()                       # the originals stay resident, same order
    cb = ix.codebook.float().numpy()
    assert (ix.codes.numpy() == SR.encode(v, a, cent, cb, ix.eta, ix.DESCENT_PASSES)).all()
    # the codes carry information: decoding them beats the centre alone
    err_c = np.linalg.norm(v - cent[a], axis=1).mean()
    err_q = np.linalg.norm(v - cent[a] - SR.decode(ix.codes.numpy(), cb), axis=1).mean()
    print("mean residual norm: centre alone", round(float(err_c), 4), "with codes", round(float(err_q), 4))
    assert err_q < 0.8 * err_c
    qv = np.random.default_rng(1).standard_normal((7, E)).astype(np.float32)
    q16 = _padded16(qv)
    for top_n in (10, 50):                                                     # below and above the reorder count (30)
        s, i, (probes, qs, rows, exact) = ix.search_device(qv, top_n, return_stages=True)
        assert probes.shape == (7, 5) and rows.shape == (7, max(top_n, 30)) and exact.shape == rows.shape
        rs, rr = SR.search(q16, cent, ix.codes.numpy(), cb, v, lb, 5, 30, top_n)
        np.testing.assert_allclose(s.numpy(), rs, atol=1e-6)
        assert (i.numpy() == np.where(rr >= 0, got_ids[np.maximum(rr, 0)], -1)).all()
        full = v.astype(np.float64) @ q16.astype(np.float64).T
        got_rows = (i.numpy() - 5) // 3
        lookup = {int(e): r for r, e in enumerate(got_ids)}
        for r in range(7):                                                     # the scores are EXACT inner products
            np.testing.assert_allclose(s.numpy()[r], [full[lookup[int(e)], r] for e in i.numpy()[r]], atol=1e-6)
    s1, i1 = ix.search(qv[0], 5)                                               # a 1-d query
    assert s1.shape == (1, 5) and i1.dtype == np.int64
    with pytest.raises(Exception):
        ix.search(qv, 5000)


def test_probing_every_leaf_with_a_full_reorder_is_the_exact_search():
    x, chunks, ids = _data(n=300, clusters=5)
    ix = _indexer(x.shape[1], scann_reorder=300)                                # leaves_to_search 100 > 17 leaves: clamped
    ix.index(ids, chunks)
    qv = np.random.default_rng(2).standard_normal((3, x.shape[1])).astype(np.float32)
    s, i, (probes, _, rows, _) = ix.search_device(qv, 20, return_stages=True)
    assert probes.shape == (3, 17) and rows.shape == (3, 300) and (rows >= 0).all()
    flat_s, flat_i = IR.topk_ip(_padded16(qv), ix.vectors.float().numpy(), 20)
    np.testing.assert_allclose(s.numpy(), flat_s, atol=1e-6)
    assert (i.numpy() == ix.ids.numpy()[flat_i]).all()


def test_save_into_a_directory_load_round_trip_and_foreign_files(tmp_path):
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    ix = _indexer(x.shape[1], scann_leaves_to_search=6)
    ix.index(ids, chunks)
    qv = np.random.default_rng(3).standard_normal((5, x.shape[1])).astype(np.float32)
    s0, i0 = ix.search(qv, 10)
    path = str(tmp_path / "scann.index")
    ix.save(path)
    assert os.path.isdir(path) and os.listdir(path) == ["scann_ip.npz"]
    ix2 = _indexer(x.shape[1], scann_leaves_to_search=6)
    ix2.load(path)                                                             # one argument, as the reference's
    for name in ("centroids", "codebook", "codes", "vectors", "ids", "list_begin"):
        assert torch.equal(getattr(ix2, name), getattr(ix, name)), name
    assert ix2.nlist == ix.nlist and ix2.eta == ix.eta
    s1, i1 = ix2.search(qv, 10)
    assert (s0 == s1).all() and (i0 == i1).all()
    # a directory written by scann (scann_config.pb + arrays) holds no archive of ours
    foreign = tmp_path / "scann_dir"
    foreign.mkdir()
    (foreign / "scann_config.pb").write_bytes(b"\x0a\x04" + bytes(32))
    with pytest.raises(NativeError, match="scann"):
        _indexer(x.shape[1]).load(str(foreign))
    with pytest.raises(NativeError, match="scann"):
        _indexer(x.shape[1]).load(str(foreign / "scann_config.pb"))           # a file, not a directory
    other = tmp_path / "other"
    other.mkdir()
    with open(other / "scann_ip.npz", "wb") as f:
        np.savez(f, magic=np.array("matchmaker_amd.IVFFlatIPIndexer"), format=np.array(1))
    with pytest.raises(NativeError, match="ScannIPIndexer file"):
        _indexer(x.shape[1]).load(str(other))
    (other / "scann_ip.npz").write_bytes(b"IwFl" + bytes(64))
    with pytest.raises(NativeError, match="ScannIPIndexer file"):
        _indexer(x.shape[1]).load(str(other))
    with pytest.raises(NativeError, match="-dim"):
        _indexer(x.shape[1] + 1).load(path)
    z = dict(np.load(os.path.join(path, "scann_ip.npz"), allow_pickle=False))
    for damage in (dict(codes=z["codes"][:-1]), dict(codes=z["codes"][:, :16]), dict(ids=z["ids"][:-1]),
                   dict(codebook=z["codebook"][:, :8]), dict(list_begin=z["list_begin"][:-1])):
        with open(other / "scann_ip.npz", "wb") as f:
            np.savez(f, **dict(z, **damage))
        with pytest.raises(NativeError, match="damaged"):
            _indexer(x.shape[1]).load(str(other))


def test_two_builds_from_one_seed_are_equal_and_the_codebook_training_is_seeded():
    from matchmaker_amd.retrieval import train_ah_codebook
    x, chunks, ids = _data()
    a, b = _indexer(x.shape[1]), _indexer(x.shape[1])
    a.index(ids, chunks)
    b.index(ids, chunks)
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.codebook, b.codebook) and torch.equal(a.codes, b.codes)
    res = torch.from_numpy(np.random.default_rng(0).standard_normal((500, 8)).astype(np.float32))
    c1, c2 = train_ah_codebook(res, 5, seed=3, chunk=128), train_ah_codebook(res, 5, seed=3, chunk=500)
    assert c1.shape == (4, 16, 2) and torch.allclose(c1, c2, atol=1e-5)
    assert not torch.equal(c1, train_ah_codebook(res, 5, seed=4))
    assert train_ah_codebook(res[:3], 2).shape == (4, 16, 2)                   # fewer rows than centres


# ---- sharded index under gloo -------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


N_SHARDED = 601                                                                # odd: uneven shards


def _exhaustive_indexer(E):
    """every leaf is probed and every row re-scored: each shard's result is its exact top-k"""
    return _indexer(E, scann_reorder=N_SHARDED)


def _scann_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from matchmaker_amd.sharding import shard_range
    x, chunks, ids = _data(n=N_SHARDED)
    ix = _exhaustive_indexer(x.shape[1])
    ix.index(ids, chunks)
    lo, hi = shard_range(N_SHARDED, world, rank)
    assert ix.vectors.shape == (hi - lo, 128) and sorted(ix.ids.tolist()) == np.concatenate(ids)[lo:hi].tolist()
    assert ix.nlist == int(np.sqrt(N_SHARDED))                                 # leaves from the whole collection
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    ix.save(os.path.join(out_dir, "scann.index"))
    np.save(os.path.join(out_dir, f"cent{rank}.npy"), ix.centroids.numpy())
    np.save(os.path.join(out_dir, f"cb{rank}.npy"), ix.codebook.numpy())
    np.save(os.path.join(out_dir, f"s{rank}.npy"), s)
    np.save(os.path.join(out_dir, f"i{rank}.npy"), i)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_sharded_search_equals_single_process(tmp_path):
    world = 2
    mp.spawn(_scann_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert (np.load(tmp_path / "cent0.npy") == np.load(tmp_path / "cent1.npy")).all()      # broadcast from rank 0
    assert (np.load(tmp_path / "cb0.npy") == np.load(tmp_path / "cb1.npy")).all()
    assert (np.load(tmp_path / "i0.npy") == np.load(tmp_path / "i1.npy")).all()
    assert sorted(os.listdir(tmp_path / "scann.index")) == ["scann_ip.npz.rank0", "scann_ip.npz.rank1"]
    x, chunks, ids = _data(n=N_SHARDED)
    ix = _exhaustive_indexer(x.shape[1])
    ix.index(ids, chunks)
    assert (ix.centroids.numpy() == np.load(tmp_path / "cent0.npy")).all()
    assert (ix.codebook.numpy() == np.load(tmp_path / "cb0.npy")).all()
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    flat_s, flat_i = IR.topk_ip(_padded16(qv), _padded16(x), 25)
    np.testing.assert_allclose(s, flat_s, atol=1e-6)                           # exhaustive: the exact top-25
    np.testing.assert_allclose(np.load(tmp_path / "s0.npy"), s, atol=1e-6)
    distinct = np.ones_like(s, bool)
    distinct[:, 1:] &= np.diff(s, axis=1) != 0
    distinct[:, :-1] &= np.diff(s, axis=1) != 0
    assert (np.load(tmp_path / "i0.npy")[distinct] == i[distinct]).all()
    assert (i[distinct] == np.concatenate(ids)[flat_i][distinct]).all()
