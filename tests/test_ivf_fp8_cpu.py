"""CPU tests of the fp8 IVF list scan and index (mm_ivf_scan_fp8_fwd, ops.ivf_scan_fp8, retrieval.IVFFp8IPIndexer,
TokenStore.build_token_index): the C ABI declaration and binding, every refusal through the raw binding (nothing is
launched), the operator's argument checks, the indexer's host logic with numpy stand-ins for the device operators, and the
preconditions of tests/test_ivf_fp8_gpu.py from the restatements alone."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import colbert_search_reference as C
from tests import fp8_store_reference as F
from tests import fp8_token_search_reference as R
from tests import ivf_fp8_reference as I8
from tests import ivf_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ C ABI and binding
def test_header_binding_and_sources_declare_the_entry():
    from matchmaker_amd import _lib, build, ops
    from tests import abi
    L = abi.assert_bound(("mm_ivf_scan_fp8_workspace_bytes", "mm_ivf_scan_fp8_fwd"))
    hdr = open(os.path.join(ROOT, "include", "mm_native.h")).read()
    section = hdr[hdr.index("fp8 IVF list scan"):]
    assert "faiss_indices.py:106-145" in section and hdr.index("fp8 IVF list scan") > hdr.index("fp8 token search")
    assert "ivf_scan_fp8.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ivf_scan_fp8.hip"))
    assert L.mm_abi_version() == 4 == _lib.ABI_VERSION
    assert callable(ops.ivf_scan_fp8)


def test_every_refusal_is_reached_before_any_launch():
    from matchmaker_amd import _lib
    L = _lib.lib()
    p = 4096                                                               # any non-null aligned value: refused before it is used
    F16, BF16, F32 = _lib.MM_F16, _lib.MM_BF16, _lib.MM_F32
    for shape in ((1000, 10, 7, 3, 10), (14906, 15, 700, 6, 1000), (1100000, 20000, 6980, 500, 1000)):
        assert L.mm_ivf_scan_fp8_workspace_bytes(*shape) == L.mm_ivf_scan_workspace_bytes(*shape) > 0
    big = 1 << 40

    def call(queries=p, codes=p, scales=p, lb=p, probes=p, n=8, nlist=3, nq=1, nprobe=2, E=128, dt=F16, k=2, out_s=p, out_r=p,
             ws=p, wsb=big):
        return L.mm_ivf_scan_fp8_fwd(queries, codes, scales, lb, probes, n, nlist, nq, nprobe, E, dt, k, out_s, out_r, ws, wsb,
                                     None)

    for kw in ({"queries": None}, {"codes": None}, {"scales": None}, {"lb": None}, {"probes": None}, {"out_s": None},
               {"out_r": None}):
        assert call(**kw) == _lib.MM_EINVAL, kw
    assert b"null pointer" in L.mm_last_error()
    for kw in ({"nlist": 0}, {"nq": 0}, {"nprobe": 0}, {"k": 0}, {"n": -1}):
        assert call(**kw) == _lib.MM_EINVAL, kw
    assert call(dt=F32) == _lib.MM_EUNSUPPORTED
    assert b"fp16 or bf16" in L.mm_last_error()
    for E in (100, 64, 640, 1024):
        assert call(E=E) == _lib.MM_EUNSUPPORTED
        assert b"pad the vectors" in L.mm_last_error()
    assert call(k=4097) == _lib.MM_EUNSUPPORTED and call(nprobe=4097) == _lib.MM_EUNSUPPORTED
    assert call(n=1 << 31) == _lib.MM_EUNSUPPORTED and call(nq=1 << 20, nprobe=4096) == _lib.MM_EUNSUPPORTED
    assert call(queries=p + 8) == _lib.MM_EINVAL and call(codes=p + 8) == _lib.MM_EINVAL and call(scales=p + 2) == _lib.MM_EINVAL
    assert b"aligned" in L.mm_last_error()
    need = L.mm_ivf_scan_fp8_workspace_bytes(8, 3, 1, 2, 2)
    assert call(wsb=need - 1) == _lib.MM_EWORKSPACE and call(ws=None) == _lib.MM_EWORKSPACE and call(wsb=16) == _lib.MM_EWORKSPACE
    for dt in (F16, BF16):                                                 # (a served dtype gets as far as the workspace check)
        assert call(dt=dt, wsb=0) == _lib.MM_EWORKSPACE
    assert call(n=0, codes=None, scales=None, wsb=0) == _lib.MM_EWORKSPACE  # an empty store needs no codes; still no launch


def test_operator_refuses_cpu_tensors_and_malformed_arguments(monkeypatch):
    from matchmaker_amd import NativeError, ops
    q = torch.zeros(2, 128, dtype=torch.float16)
    codes, scales = torch.zeros(8, 128, dtype=torch.uint8), torch.ones(8)
    lb, pr = torch.tensor([0, 4, 8]), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(NativeError, match="CPU tensor"):
        ops.ivf_scan_fp8(q, codes, scales, lb, pr, 2)
    # the argument checks themselves, on meta tensors (the device check is stepped over: a meta tensor is no HIP tensor)
    monkeypatch.setattr(ops, "_dev_check", lambda *ts: torch.device("meta"))
    m = dict(device="meta")
    qm = torch.empty(2, 128, dtype=torch.float16, **m)
    cm, sm = torch.empty(8, 128, dtype=torch.uint8, **m), torch.empty(8, dtype=torch.float32, **m)
    lbm, prm = torch.empty(3, dtype=torch.int64, **m), torch.empty(2, 1, dtype=torch.int32, **m)
    bad = [
        ((qm.float(), cm, sm, lbm, prm, 2), "fp16 or bf16"),                                  # dot_topk_fp8's refusals
        ((qm.to(torch.int32), cm, sm, lbm, prm, 2), "queries: expected"),
        ((qm[0], cm, sm, lbm, prm, 2), "queries: expected"),
        ((qm, cm.to(torch.int8), sm, lbm, prm, 2), "codes: expected"),
        ((qm, cm[0], sm, lbm, prm, 2), "codes: expected"),
        ((qm, cm, sm.double(), lbm, prm, 2), "scales: expected"),
        ((qm, cm, sm[:7], lbm, prm, 2), "scales: expected"),
        ((qm, cm[:, :64], sm, lbm, prm, 2), "dims differ: 128 vs 64"),
        ((torch.empty(2, 64, dtype=torch.float16, **m), cm[:, :64], sm, lbm, prm, 2), "pad the vectors"),
        ((qm, cm, sm, lbm.int(), prm, 2), "list_begin"),                                      # ivf_scan's refusals
        ((qm, cm, sm, lbm[:1], prm, 2), "list_begin"),
        ((qm, cm, sm, lbm, prm.long(), 2), "probes"),
        ((qm, cm, sm, lbm, torch.empty(3, 1, dtype=torch.int32, **m), 2), "probes"),
        ((qm, cm, sm, lbm, torch.empty(2, 0, dtype=torch.int32, **m), 2), "probes"),
        ((qm, cm, sm, lbm, prm, 0), "outside 1 .. 4096"),
        ((qm, cm, sm, lbm, prm, 4097), "outside 1 .. 4096"),
        ((qm, cm, sm, lbm, torch.empty(2, 4097, dtype=torch.int32, **m), 2), "outside 1 .. 4096"),
    ]
    for args, what in bad:
        with pytest.raises(NativeError, match=what):
            ops.ivf_scan_fp8(*args)
    s, r = ops.ivf_scan_fp8(qm[:0], cm, sm, lbm, prm[:0], 3)                                  # nq == 0: no call
    assert s.shape == (0, 3) and r.shape == (0, 3) and r.dtype == torch.int64


# ------------------------------------------------------------------------------------------ the indexer through stand-ins
def _topk_fn(q, c, k):
    s, i = IR.topk_ip(q.float().numpy(), c.float().numpy(), k)
    return torch.from_numpy(s), torch.from_numpy(i)


def _scan_fn(q, codes, scales, lb, probes, k):
    assert codes.dtype == torch.uint8 and scales.dtype == torch.float32 and scales.shape == (codes.shape[0],)
    s, r = I8.ivf_scan_fp8(q.float().numpy(), codes.numpy(), scales.numpy(), lb.numpy(), probes.numpy(), k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(r)


def _merge_fn(s, ids, k):
    s = s.clone()
    s[ids < 0] = float("-inf")
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(s, 1, order), torch.gather(ids, 1, order)


_FNS = {"topk_fn": _topk_fn, "scan_fn": _scan_fn, "merge_fn": _merge_fn, "quantize_fn": F.quantize_torch}


def _indexer(E, nlist, nprobe, **kw):
    from matchmaker_amd.retrieval import IVFFp8IPIndexer
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": nprobe}
    return IVFFp8IPIndexer(cfg, device="cpu", **_FNS, **kw)


def _flat_indexer(E, nlist, nprobe):
    from matchmaker_amd.retrieval import IVFFlatIPIndexer
    from tests.test_ivf_cpu import _scan_fn as scan16
    cfg = {"token_dim": E, "faiss_ivf_list_count": nlist, "faiss_ivf_search_probe_count": nprobe}
    return IVFFlatIPIndexer(cfg, device="cpu", topk_fn=_topk_fn, scan_fn=scan16, merge_fn=_merge_fn)


def _data(n=600, E=40, clusters=12, seed=5):
    x, _ = IR.clustered(n, E, clusters, seed)
    chunks = [x[: n // 3], x[n // 3:]]
    ids = [np.arange(0, n // 3, dtype=np.int64) * 3 + 5, np.arange(n // 3, n, dtype=np.int64) * 3 + 5]
    return x, chunks, ids


def _padded16(x, E_pad=128):
    xp = np.zeros((x.shape[0], E_pad), np.float16)
    xp[:, : x.shape[1]] = x.astype(np.float16)
    return xp


def test_index_layout_ids_and_search_against_the_restatement():
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    n, E, nlist = x.shape[0], x.shape[1], 16
    ix = _indexer(E, nlist, 4)
    ix.prepare(chunks)                                                     # inherited: 16-bit training vectors
    assert ix.centroids.shape == (nlist, 128) and ix.centroids.dtype == torch.float16
    ix.index(ids, chunks)
    assert ix.codes.shape == (n, 128) and ix.codes.dtype == torch.uint8
    assert ix.scales.shape == (n,) and ix.scales.dtype == torch.float32
    with pytest.raises(NativeError, match=r"\.codes / \.scales"):
        ix.vectors
    lb = ix.list_begin.numpy()
    cent = ix.centroids.float().numpy()
    # the lists hold the quantised rows of the input, under one permutation with the ids, input order inside a list
    got_ids = ix.ids.numpy()
    assert sorted(got_ids.tolist()) == sorted(np.concatenate(ids).tolist())
    want_c, want_s = F.quantize_torch(torch.from_numpy(_padded16(x)))
    src = (got_ids - 5) // 3
    assert np.array_equal(ix.codes.numpy(), want_c.numpy()[src]) and np.array_equal(ix.scales.numpy(), want_s.numpy()[src])
    for l in range(nlist):
        assert (np.diff(got_ids[lb[l]: lb[l + 1]]) > 0).all()
    # one assignment rule: the best centroid of the value the index stores, deq(code) * scale as float16
    v = F.dequantize_torch(ix.codes, ix.scales, torch.float16).float().numpy()
    a = IR.assign(v, cent)
    assert (np.diff(a) >= 0).all() and lb[0] == 0 and lb[-1] == n
    assert (np.diff(lb) == np.bincount(a, minlength=nlist)).all()
    # search = probe selection on the 16-bit centroids + the restated scan of the probed lists, mapped to external ids
    qv = np.random.default_rng(1).standard_normal((7, E)).astype(np.float32)
    s, i, probes = ix.search_device(qv, 20, return_probes=True)
    assert probes.shape == (7, 4) and probes.dtype == torch.int32
    q16 = np.zeros((7, 128), np.float32)
    q16[:, :E] = qv.astype(np.float16)
    ref_p = IR.topk_ip(q16, cent, 4)[1]
    assert (probes.numpy() == ref_p).all()
    ref_s, ref_r = I8.ivf_scan_fp8(q16, ix.codes.numpy(), ix.scales.numpy(), lb, ref_p, 20)
    assert np.array_equal(s.numpy(), ref_s.astype(np.float32))
    assert (i.numpy() == np.where(ref_r >= 0, got_ids[np.maximum(ref_r, 0)], -1)).all()
    s1, i1 = ix.search(qv[0], 5)                                                              # a 1-d query
    assert s1.shape == (1, 5) and (i1[0] == i.numpy()[0, :5]).all()


def test_index_resident_and_index_codes_build_bit_equal_indices_and_train_codes_is_seeded():
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    xp = torch.from_numpy(_padded16(x))
    all_ids = torch.from_numpy(np.concatenate(ids))
    a, b = _indexer(x.shape[1], 16, 4), _indexer(x.shape[1], 16, 4)
    a.prepare(chunks)
    b.centroids = a.centroids.clone()
    a.index_resident(all_ids, xp)
    b.DEQ_CHUNK = 256                                                      # several chunks, one of them partial
    b.index_codes(all_ids, *F.quantize_torch(xp))
    for f in ("codes", "scales", "ids", "list_begin"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    # train_codes: a seeded sample of the rows, dequantised to float16; two runs from one seed agree
    codes, scales = F.quantize_torch(xp)
    c, d = _indexer(x.shape[1], 8, 2), _indexer(x.shape[1], 8, 2)
    c.train_codes(codes, scales, subsample=0.5)
    d.DEQ_CHUNK = 100
    d.train_codes(codes, scales, subsample=0.5)
    assert torch.equal(c.centroids, d.centroids) and c.centroids.dtype == torch.float16
    e = _indexer(x.shape[1], 8, 2)
    e.train_resident(F.dequantize_torch(codes, scales, torch.float16), subsample=0.5)
    assert torch.equal(c.centroids, e.centroids)                           # = training on the values the codes hold
    with pytest.raises(NativeError, match="training vectors"):
        _indexer(x.shape[1], 64, 2).train_codes(codes[:60], scales[:60])
    # refusals: another width, other dtypes, ids of another length, no centroids yet
    for bad in ((codes[:, :64].contiguous(), scales), (codes.to(torch.int8), scales), (codes, scales.double()), (codes, scales[:-1])):
        with pytest.raises(NativeError, match="need uint8"):
            a.index_codes(all_ids, *bad)
        with pytest.raises(NativeError, match="need uint8"):
            a.train_codes(*bad)
    with pytest.raises(NativeError, match="ids for"):
        a.index_codes(all_ids[:-1], codes, scales)
    with pytest.raises(NativeError, match="first"):
        _indexer(x.shape[1], 16, 4).index_codes(all_ids, codes, scales)
    with pytest.raises(NativeError, match="no 16-bit rows"):
        a.vectors = xp


def test_empty_list_clamped_nprobe_and_padding():
    x, chunks, ids = _data(n=300, clusters=5)
    ix = _indexer(x.shape[1], 8, 100)                          # nprobe > nlist: clamped
    ix.prepare(chunks)
    ix.index(ids, chunks)
    lb = ix.list_begin.clone()
    l = int(torch.diff(lb).argmax())                           # empty one list by hand
    keep = torch.ones(lb[-1].item(), dtype=torch.bool)
    keep[lb[l]: lb[l + 1]] = False
    removed = int((~keep).sum())
    ix.codes, ix.scales, ix.ids = ix.codes[keep], ix.scales[keep], ix.ids[keep]
    lb[l + 1:] -= removed
    ix.list_begin = lb
    assert lb[l] == lb[l + 1]
    qv = np.random.default_rng(2).standard_normal((3, x.shape[1])).astype(np.float32)
    n_left = 300 - removed
    s, i, probes = ix.search_device(qv, n_left + 7, return_probes=True)
    assert probes.shape == (3, 8)                              # every list probed: the search is exhaustive
    assert (i[:, n_left:] == -1).all() and torch.isneginf(s[:, n_left:]).all()
    assert (i[:, :n_left] >= 0).all() and torch.isfinite(s[:, :n_left]).all()
    q16 = np.pad(qv.astype(np.float16).astype(np.float32), ((0, 0), (0, 128 - x.shape[1])))
    flat_s, flat_i = R.dot_topk_fp8_exact(q16, ix.codes.numpy(), ix.scales.numpy(), n_left)
    assert np.array_equal(s[:, :n_left].numpy(), flat_s.astype(np.float32))
    assert (i[:, :n_left].numpy() == ix.ids.numpy()[flat_i]).all()


def test_save_load_round_trip_probe_overwrite_and_the_cross_class_refusals(tmp_path):
    from matchmaker_amd import NativeError
    x, chunks, ids = _data()
    ix = _indexer(x.shape[1], 16, 3)
    ix.prepare(chunks)
    ix.index(ids, chunks)
    qv = np.random.default_rng(3).standard_normal((5, x.shape[1])).astype(np.float32)
    s0, i0 = ix.search(qv, 10)
    path = str(tmp_path / "ivf_fp8.index")
    ix.save(path)
    z = np.load(path, allow_pickle=False)
    assert str(z["magic"]) == "matchmaker_amd.IVFFp8IPIndexer" and int(z["format"]) == 1 and "vectors" not in z.files
    assert z["codes"].dtype == np.uint8 and z["scales"].dtype == np.float32
    ix2 = _indexer(x.shape[1], 16, 3)
    ix2.load(path)
    for f in ("centroids", "codes", "scales", "ids", "list_begin"):
        assert torch.equal(getattr(ix, f), getattr(ix2, f)), f
    s1, i1 = ix2.search(qv, 10)
    assert (s0 == s1).all() and (i0 == i1).all()
    ix3 = _indexer(x.shape[1], 16, 3)
    ix3.load(path, config_overwrites={"faiss_ivf_search_probe_count": 16})
    assert ix3.nprobe == 16 and ix3.search_device(qv, 10, return_probes=True)[2].shape == (5, 16)
    # the two IVF classes refuse each other's archives, by the name of the class that wrote the file
    with pytest.raises(NativeError, match="written by IVFFp8IPIndexer"):
        _flat_indexer(x.shape[1], 16, 3).load(path)
    flat = _flat_indexer(x.shape[1], 16, 3)
    flat.prepare(chunks)
    flat.index(ids, chunks)
    path16 = str(tmp_path / "ivf.index")
    flat.save(path16)
    with pytest.raises(NativeError, match="written by IVFFlatIPIndexer"):
        _indexer(x.shape[1], 16, 3).load(path16)
    flat2 = _flat_indexer(x.shape[1], 16, 3)
    flat2.load(path16)                                                     # (and each still reads its own)
    assert torch.equal(flat2.vectors, flat.vectors)
    bogus = tmp_path / "faiss.index"
    bogus.write_bytes(b"IwFl" + bytes(64))
    with pytest.raises(NativeError, match="faiss"):
        _indexer(x.shape[1], 16, 3).load(str(bogus))


# ---- sharded under gloo ---------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from matchmaker_amd.sharding import shard_range
    x, chunks, ids = _data(n=601)                               # odd size: uneven shards
    ix = _indexer(x.shape[1], 16, 5)
    ix.prepare(chunks)
    ix.index(ids, chunks)
    lo, hi = shard_range(601, world, rank)
    assert ix.codes.shape == (hi - lo, 128) and sorted(ix.ids.tolist()) == np.concatenate(ids)[lo:hi].tolist()
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    ix.save(os.path.join(out_dir, "ivf_fp8.index"))
    np.save(os.path.join(out_dir, f"cent{rank}.npy"), ix.centroids.numpy())
    np.save(os.path.join(out_dir, f"s{rank}.npy"), s)
    np.save(os.path.join(out_dir, f"i{rank}.npy"), i)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_sharded_index_equals_single_process(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    c0, c1 = np.load(tmp_path / "cent0.npy"), np.load(tmp_path / "cent1.npy")
    assert (c0 == c1).all()
    assert (np.load(tmp_path / "i0.npy") == np.load(tmp_path / "i1.npy")).all()
    assert os.path.exists(tmp_path / "ivf_fp8.index.rank0") and os.path.exists(tmp_path / "ivf_fp8.index.rank1")
    x, chunks, ids = _data(n=601)
    ix = _indexer(x.shape[1], 16, 5)
    ix.prepare(chunks)
    assert (ix.centroids.numpy() == c0).all()
    ix.index(ids, chunks)
    qv = np.random.default_rng(4).standard_normal((6, x.shape[1])).astype(np.float32)
    s, i = ix.search(qv, 25)
    assert np.array_equal(np.load(tmp_path / "s0.npy"), s)      # per-row quantisation: a row's value does not depend on its shard
    distinct = np.ones_like(s, bool)
    distinct[:, 1:] &= np.diff(s, axis=1) != 0
    distinct[:, :-1] &= np.diff(s, axis=1) != 0
    assert (np.load(tmp_path / "i0.npy")[distinct] == i[distinct]).all()


# ------------------------------------------------------------------------------------------ TokenStore.build_token_index
def _exact_stores():
    from matchmaker_amd.token_store import TokenStore
    c = C.exact_case()
    ids = [f"doc{i}" for i in range(len(c["begin"]))]

    def topk_fp8(q, codes, scales, k):
        s, i = R.dot_topk_fp8_exact(q.double().numpy(), codes.numpy(), scales.numpy(), k)
        return torch.from_numpy(s).float(), torch.from_numpy(i)

    st = TokenStore(torch.from_numpy(c["tokens"]).half(), ids, c["begin"], c["end"], topk_fn=_topk_fn, merge_fn=_merge_fn,
                    quantize_fn=F.quantize_torch, topk_fp8_fn=topk_fp8)
    return c, st, st.quantize_fp8()


def test_build_token_index_picks_the_class_and_its_hits_equal_the_flat_fp8_search():
    from matchmaker_amd import NativeError
    from matchmaker_amd.retrieval import IVFFlatIPIndexer, IVFFp8IPIndexer
    from tests.test_ivf_cpu import _scan_fn as scan16
    c, st, f8 = _exact_stores()
    T = c["tokens"].shape[0]
    cfg = {"faiss_ivf_list_count": 8, "faiss_ivf_search_probe_count": 8}
    ix = f8.build_token_index(cfg, native_kmeans=False, **_FNS)
    assert type(ix) is IVFFp8IPIndexer and ix.token_dim == 128 and "token_dim" not in cfg
    assert sorted(ix.ids.tolist()) == list(range(T))                       # ids = token rows
    assert torch.equal(ix.codes, f8.codes[ix.ids]) and torch.equal(ix.scales, f8.scales[ix.ids])
    with pytest.raises(NativeError, match="16-bit rows are not resident"):
        f8.tokens                                                          # fp8-ONLY: nothing 16-bit was needed
    ix16 = st.build_token_index(cfg, native_kmeans=False, topk_fn=_topk_fn, scan_fn=scan16, merge_fn=_merge_fn,
                                quantize_fn=F.quantize_torch)
    assert type(ix16) is IVFFlatIPIndexer and sorted(ix16.ids.tolist()) == list(range(T))
    assert torch.equal(ix16.vectors, st.tokens[ix16.ids])
    # every list probed: the same k' rows per live token as the brute-force search of the codes.  The scan orders equal
    # scores by the row of its list-ordered copy and the flat search by token row, so a tie may come out in another order
    # (and, at the k'-th score, as another member of the tie): the SCORES of the hits are compared, and the rows wherever
    # the score is not tied at the cut.
    q = torch.from_numpy(c["q"])
    k = c["k"]
    flat = f8.token_hits(q, k, token_search="fp8").view(-1, k).numpy()
    got = f8.token_hits(q, k, index=ix).view(-1, k).numpy()
    full = R.scores64(c["q"].reshape(-1, 128), f8.codes.numpy(), f8.scales.numpy())
    dead = ~(c["q"].reshape(-1, 128) != 0).any(axis=1)
    assert dead.sum() == 10 and (got[dead] == -1).all() and (flat[dead] == -1).all()
    n_equal = 0
    for t in np.nonzero(~dead)[0]:
        assert len(set(got[t].tolist())) == k and (got[t] >= 0).all()
        sg, sf = np.sort(full[t, got[t]]), np.sort(full[t, flat[t]])
        assert np.array_equal(sg, sf), t
        above = full[t] > sf[0]                                            # strictly above the k'-th score: in both sets
        assert set(np.nonzero(above)[0].tolist()) <= set(got[t].tolist())
        n_equal += int(np.array_equal(np.sort(got[t]), np.sort(flat[t])))
    assert n_equal >= 0.9 * (~dead).sum()
    # a store whose width is no native width is refused by name
    from matchmaker_amd.token_store import TokenStore
    small = TokenStore(torch.zeros(4, 16, dtype=torch.float16) + 1, ["a"], [0], [4])
    with pytest.raises(NativeError, match="pad the rows"):
        small.build_token_index(cfg)


# ------------------------------------------------------------------------------------------ preconditions of the GPU tests
@pytest.mark.parametrize("E,nq,k", I8.EXACT)
def test_exact_cases_are_exact_in_fp32_and_hold_ties(E, nq, k):
    """(a) every score of the scaled store is an integer multiple of 1/8 below 2^24 eighths: any summation order is exact in
    fp32.  From the value ranges for every case; numerically, with the ties, on up to 37 queries of it."""
    q, codes, scales, lb, probes = I8.exact_problem(E, nq, I8.EXACT_NPROBE, I8.exact_seed(E, nq, k))
    vals = F.deq_numpy(codes)
    assert codes.shape == (I8.N_ROWS, E) and lb[-1] == I8.N_ROWS == 14906
    assert np.abs(vals).max() <= 8 and np.array_equal(vals, np.round(vals)) and np.abs(q).max() <= 2
    assert np.array_equal(q, np.round(q)) and set(np.log2(scales).tolist()) <= set(range(-3, 4))
    assert E * 2 * 8 * 8 * 8 < 2 ** 24                                     # sum |q| |deq| * scale, in eighths
    for dt in (torch.float16, torch.bfloat16):
        assert np.array_equal(torch.from_numpy(q).to(dt).float().numpy(), q)
    assert probes[0].tolist() == [8, -1, 5, 3, -1, -1] and all(len(set(p[p >= 0].tolist())) == (p >= 0).sum() for p in probes)
    n = min(nq, 37)
    full = R.scores64(q[:n], codes, scales)
    assert np.array_equal(full * 8, np.round(full * 8)) and R.magnitudes64(q[:n], codes, scales).max() * 8 < 2 ** 24
    s, r = I8.ivf_scan_fp8(q[:n], codes, scales, lb, probes[:n], k, full=full)
    assert all((np.diff(s[i][np.isfinite(s[i])]) <= 0).all() for i in range(n))
    ties_inside = sum(int((np.diff(s[i][np.isfinite(s[i])]) == 0).sum()) for i in range(n))
    at_cut = 0
    for i in range(n):
        union = IR.union_rows(lb, probes[i])
        if union.size > k:
            at_cut += int((full[i, union] == s[i, k - 1]).sum() >= 2)
    print(f"E {E} nq {nq} k {k}: equal neighbours inside the lists {ties_inside}, queries with a tie group at the k-th score {at_cut} of {n}")
    assert ties_inside > 0 or k == 1
    if k == 10 and nq > 1:                                                 # (k = 1: the best score is rarely tied; k = 1000: a sparse tail)
        assert at_cut > 0


def test_tie_problem_keeps_its_40_ties_from_rank_8_when_quantised():
    q, codes, scales, lb, probes, k, group = I8.tie_problem()
    assert (codes[group] == codes[group[0]]).all() and (scales[group] == scales[group[0]]).all()
    _, v, _, _, _, _ = IR.tie_problem()
    assert np.array_equal(F.dequantize_numpy(codes, scales), v)            # the quantisation is exact: the scores are the 16-bit ones
    ref_s, ref_r = I8.ivf_scan_fp8(q, codes, scales, lb, probes, k)
    full = R.scores64(q, codes, scales)
    for i in range(q.shape[0]):                                            # the restatement against a plain (score, row) sort
        rows = IR.union_rows(lb, probes[i])
        order = np.lexsort((rows, -full[i, rows]))[:k]
        assert np.array_equal(ref_r[i], rows[order]) and np.array_equal(ref_s[i], full[i, rows][order])
    assert ref_s[0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0, 0, 0] and ref_r[0, 7:].tolist() == group[:3].tolist()
    assert (full[0, IR.union_rows(lb, probes[0])] == 0).sum() == 40


def test_short_union_case_finds_16_0_17_31_0():
    lb = I8.list_begin()
    assert [IR.union_rows(lb, p).size for p in I8.short_union_probes()] == I8.SHORT_FOUND


def test_the_end_to_end_store_is_clear_at_the_cut():
    """(b) the random-normal store of the end-to-end GPU test: for every live token score_16 - score_17 in float64 exceeds the
    two scores' (E + 2) 2^-24 scale sum |q| |deq| bounds together, so the IVF scan and the flat search, which sum in different
    orders, return the same 16 rows."""
    tight, conservative = I8.normal_store_gap_over_bound()
    print(f"seed {I8.NORMAL_SEED}: smallest gap / (bound_16 + bound_17) = {tight:.2f}; / (2 x largest bound) = {conservative:.2f}")
    assert conservative > 1.0 and tight > 1.0
