"""Drop-ins for matchmaker's GPU faiss indices on MI355X.  FlatIPIndexer (brute force): same surface as
`FaissIdIndexer` (matchmaker/retrieval/faiss_indices.py:49-74; base class :13-36) —
`prepare(data_chunks)`, `index(ids, data_chunks)`, `search(query_vec, top_n) -> (scores, ids)` —
with the collection resident in HBM as float16 (what `co.useFloat16` stores on the reference's GPUs)
and the search done by the native Q x C^T + exact top-k kernels (mm_dot_topk_fwd).

Multi-GPU = the reference's `co.shard = True` (:62-66): every rank holds a contiguous shard of the
vectors; `search` runs the local top-k, all-gathers the [nq, k] (score, id) lists over RCCL and
merges them natively (mm_topk_merge).  Used from dense_retrieval.py:308-328 (construction),
:333-336 (prepare / index) and :391 (search).

IVFFlatIPIndexer (faiss_index_type: ivf) has the surface of `FaissIVFIndexer` (faiss_indices.py:106-145): spherical
k-means centroids, the shard stored list by list, probe selection with the same top-k kernel and the exact scan of
the probed lists by mm_ivf_scan_fwd.

IVFFp8IPIndexer is IVFFlatIPIndexer with the lists held as the fp8 token store holds its rows (e4m3fn codes + one power-of-two
scale per row) and scanned by mm_ivf_scan_fp8_fwd: the token index of an fp8-only ColBERT store at half the bytes.

DynamicIVFIndexer has the surface of `FaissDynamicIndexer` (faiss_indices.py:307-428), the index behind TAS-Balanced query
clustering (matchmaker/distillation/query_clusterer.py:187-221): k-means over the query vectors, one probe, entries that
can be replaced.  Its k-means (`spherical_kmeans`) runs on mm_kmeans_assign / mm_kmeans_segment_sum; IVFFlatIPIndexer
takes the same path with `native_kmeans=True`.

GraphIPIndexer (faiss_index_type: hnsw) has the surface of `FaissHNSWIndexer` (a CPU index in the reference): a one-level
neighbour graph built exactly from the shard's k-NN lists (the top-k kernel over the shard itself), searched by
mm_graph_search_fwd from entry rows that the top-k kernel picks out of a strided sample.

ScannIPIndexer (faiss_index_type: scann) has the surface of `ScaNNIndexer` (matchmaker/retrieval/scann_index.py:10-53, a CPU
library in the reference): int(sqrt(n)) spherical k-means leaves, 4-bit anisotropic codes of 2-dimensional blocks of the
residuals (mm_ah_encode), probe selection with the top-k kernel, the scan of the probed leaves' codes (mm_ah_scan_fwd) and
the exact re-score of the best candidates from the resident originals (mm_gather_dot).

MaxPIndexer wraps any of them for document retrieval over a passage index (`maxP->bert_dot`, dense_retrieval.py:414-429): the
inner index returns passage hits under repeated document ids and ops.distinct_hits keeps the first hit of every document.

What the indexers have in common lives once, in two private bases: `_DeviceIndex` (the config and device set-up with the
float16 refusal, the chunk-by-chunk copy to the device, rows -> ids) and, for the four that shard over a process group,
`_ShardedIndex` (this rank's shard, the resident-shard check, `search()`, the all-gather + merge, the archive writer and
reader).  A class keeps what is its own: training, layout, `search_device`, the fields of its archive.
"""
import os
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .sharding import shard_range


def _pad_dim(E: int) -> int:
    for e in (128, 256, 384, 512, 768):
        if E <= e:
            return e
    raise ops.NativeError(f"token_dim {E} > 768 is not supported by the native flat index")


def _device_queries(query_vec, dtype, E_pad: int, token_dim: int, device) -> torch.Tensor:
    """The queries as the index stores its vectors: [nq, E_pad] `dtype` on `device` (a single vector becomes one row;
    a tensor that already has that form is used as it is)."""
    q = torch.as_tensor(query_vec)
    if q.dim() == 1:
        q = q[None, :]
    if q.is_cuda and q.dtype == dtype and q.shape[1] == E_pad and q.is_contiguous():
        return q
    qd = torch.zeros((q.shape[0], E_pad), dtype=dtype, device=device)
    qd[:, : token_dim] = q.to(device).to(dtype)
    return qd


def _unit_rows(c: torch.Tensor) -> torch.Tensor:
    return c / c.norm(dim=1, keepdim=True).clamp_min(1e-20)


def _lists_of(a: torch.Tensor, nlist: int):
    """An assignment [n] -> (order [n] int64 = the rows list by list, input order inside a list; list_begin [nlist + 1]
    int64; counts [nlist] int64)."""
    a = a.to(torch.int64)
    order = torch.sort(a, stable=True).indices
    counts = torch.bincount(a, minlength=nlist)
    lb = torch.zeros(nlist + 1, dtype=torch.int64, device=a.device)
    lb[1:] = torch.cumsum(counts, 0)
    return order, lb, counts


def spherical_kmeans(x: torch.Tensor, nlist: int, iters: int = 20, seed: int = 208973249, init: Optional[torch.Tensor] = None,
                     assign_fn=None, sum_fn=None) -> torch.Tensor:
    """Spherical k-means for inner-product lists: -> centroids [nlist, E_pad] float16 of unit length.

    x [n, E] float16 (zero-padded to E_pad here when E is not one of the native widths).  The start is `init`
    ([nlist, E_pad]) when given, else a sample of nlist rows drawn with `seed`; every iteration assigns each row to its
    maximum-inner-product centroid (ops.kmeans_assign: lowest centroid on equal scores), sums the rows of every list in
    fp32 (ops.kmeans_segment_sum over a stable sort of the assignment: no atomics) and normalises the sums; an empty
    cluster is re-seeded from a vector of the largest one.  Every step is a pure function of its inputs, so two runs from
    one seed give bit-equal centroids.  assign_fn(x, centroids) -> (list, score) / sum_fn(x, order, list_begin) -> sums
    default to the native operators; the CPU test-suite injects stand-ins."""
    assign_fn = assign_fn if assign_fn is not None else ops.kmeans_assign
    sum_fn = sum_fn if sum_fn is not None else ops.kmeans_segment_sum
    if x.dim() != 2 or x.dtype != torch.float16:
        raise ops.NativeError(f"spherical_kmeans: expected float16 [n, E], got {x.dtype} {tuple(x.shape)}")
    E_pad = _pad_dim(x.shape[1])
    if x.shape[1] != E_pad:
        x = torch.nn.functional.pad(x, (0, E_pad - x.shape[1]))
    x = x.contiguous()
    n = x.shape[0]
    if not 1 <= nlist <= n:
        raise ops.NativeError(f"spherical_kmeans: {n} training vectors for {nlist} centroids")
    if init is None:
        gen = torch.Generator().manual_seed(int(seed))
        init = _unit_rows(x[torch.randperm(n, generator=gen)[:nlist].to(x.device)].float())
    elif tuple(init.shape) != (nlist, E_pad):
        raise ops.NativeError(f"spherical_kmeans: init must be [{nlist}, {E_pad}], got {tuple(init.shape)}")
    cent = init.to(device=x.device, dtype=torch.float16).contiguous()
    for _ in range(iters):
        a = assign_fn(x, cent)[0]
        order, lb, counts = _lists_of(a, nlist)
        sums = sum_fn(x, order, lb)
        empty = torch.nonzero(counts == 0).flatten()
        if empty.numel():
            big = int(counts.argmax())
            members = order[lb[big]: lb[big + 1]]                 # ascending rows of the largest cluster
            sums[empty] = x[members[torch.arange(empty.numel(), device=x.device) % members.numel()]].float()
        cent = _unit_rows(sums).to(torch.float16).contiguous()
    return cent


def _assign_by_topk(topk_fn, x: torch.Tensor, centroids: torch.Tensor, chunk: int, out_dtype) -> torch.Tensor:
    """[n] out_dtype: the centroid of maximum inner product of every row of x, by top-1 calls of `chunk` rows (the chunk
    bounds the top-k workspace)."""
    out = torch.empty(x.shape[0], dtype=out_dtype, device=x.device)
    for a in range(0, x.shape[0], chunk):
        out[a: a + chunk] = topk_fn(x[a: a + chunk], centroids, 1)[1][:, 0]
    return out


class _DeviceIndex:
    """What every indexer of this module is: float16 vectors of `token_dim` columns, zero-padded to the native width
    `E_pad`, resident on one device, with external int64 `ids` beside them."""

    def _configure(self, config, device, refusal: str, fp16_override: bool = True):
        """base_index.py:14 derives fp16 storage from config["token_dtype"] == "float16"; `faiss_use_fp16` (not a reference
        key) is an explicit override where fp16_override is set.  faiss keeps fp32 vectors AND fp32 queries when
        useFloat16 is off (faiss_indices.py:58-61); these indices store fp16 vectors and round the queries to fp16 as well,
        so near-tie rankings could differ from an fp32 index: `refusal` is raised instead of silently changing the
        arithmetic."""
        self.token_dim = config["token_dim"]
        self.use_fp16 = config.get("token_dtype", "float16") == "float16"
        if fp16_override:
            self.use_fp16 = config.get("faiss_use_fp16", self.use_fp16)
        if not self.use_fp16:
            raise ops.NativeError(refusal)
        self.dtype = torch.float16
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())  # noqa: E501
        self.E_pad = _pad_dim(self.token_dim)

    def _to_device(self, data_chunks: List[np.ndarray], lo: int, hi: int) -> torch.Tensor:
        """Rows lo .. hi of the concatenated chunks as [hi - lo, E_pad] on the device, chunk by chunk: no second host copy."""
        vec = torch.zeros((hi - lo, self.E_pad), dtype=self.dtype, device=self.device)
        off = 0
        for c in data_chunks:
            a, b = max(lo, off), min(hi, off + c.shape[0])
            if a < b:
                vec[a - lo: b - lo, : self.token_dim] = torch.from_numpy(np.ascontiguousarray(c[a - off: b - off])).to(
                    self.device).to(self.dtype)
            off += c.shape[0]
        return vec

    def _ids_of(self, rows: torch.Tensor) -> torch.Tensor:
        """Rows of `vectors` -> external ids (IndexIDMap); -1 stays -1, and an empty shard has only those."""
        return torch.where(rows >= 0, self.ids[rows.clamp(min=0)], rows) if self.ids.numel() else rows


class _ShardedIndex(_DeviceIndex):
    """The reference's `co.shard = True` (faiss_indices.py:62-66): every rank of `group` holds a contiguous shard of the
    vectors, searches it and the ranks' lists are merged.  A subclass provides `search_device` and `_merge`."""

    merge_single_rank = False     # run the all-gathers + the merge even in a group of ONE rank (FlatIPIndexer's rehearsal)

    def _configure(self, config, device, group, refusal: str, fp16_override: bool = True):
        super()._configure(config, device, refusal, fp16_override)
        self.group = group

    def _world(self):
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.group), dist.get_rank(self.group)
        return 1, 0

    def _broadcast(self, *tensors):
        """What rank 0 of the group trained goes to the buffers the other ranks allocated."""
        if self._world()[0] > 1:
            src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
            for t in tensors:
                dist.broadcast(t, src=src, group=self.group)

    def _shard(self, ids: List[np.ndarray], data_chunks: List[np.ndarray]):
        """(ids [n_local] int64, vectors [n_local, E_pad]) of this rank's contiguous shard, on the device (every rank is
        given the same full lists, as the reference's single process is)."""
        i = np.concatenate(ids).astype(np.int64)
        lo, hi = shard_range(i.shape[0], *self._world())
        return torch.from_numpy(i[lo:hi]).to(self.device), self._to_device(data_chunks, lo, hi)

    def _check_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        if vectors.dtype != self.dtype or vectors.dim() != 2 or vectors.shape[1] != self.E_pad or ids.shape[0] != vectors.shape[0]:
            raise ops.NativeError(f"index_resident: need float16 [n, {self.E_pad}] vectors and [n] ids")

    def search(self, query_vec, top_n: int):
        """faiss_indices.py:29-36: (scores [nq, top_n] float32 descending, ids [nq, top_n] int64; -inf / -1 where the index
        reached fewer than top_n vectors) as numpy arrays."""
        s, ids = self.search_device(query_vec, top_n)
        return s.cpu().numpy(), ids.cpu().numpy()

    def _finish(self, s: torch.Tensor, ids: torch.Tensor, top_n: int):
        """co.shard's final step: all-gather every rank's [nq, top_n] (score, id) lists and merge them; one rank (and no
        rehearsal asked for) returns its own lists."""
        if not (dist.is_available() and dist.is_initialized()):
            return s, ids
        world = dist.get_world_size(self.group)
        if world > 1 or self.merge_single_rank:
            nq = s.shape[0]
            gs = torch.empty((world * nq, top_n), dtype=s.dtype, device=s.device)        # rank-major concatenation
            gi = torch.empty((world * nq, top_n), dtype=ids.dtype, device=ids.device)
            dist.all_gather_into_tensor(gs, s.contiguous(), group=self.group)             # RCCL over xGMI
            dist.all_gather_into_tensor(gi, ids.contiguous(), group=self.group)
            s, ids = self._merge(gs.view(world, nq, top_n).permute(1, 0, 2).reshape(nq, -1),
                                 gi.view(world, nq, top_n).permute(1, 0, 2).reshape(nq, -1), top_n)
        return s, ids

    def _rank_path(self, path: str) -> str:
        world, rank = self._world()
        return path if world == 1 else f"{path}.rank{rank}"

    def _write_archive(self, p: str, magic: str, fmt: int, **fields):
        """One numpy .npz archive: magic, format, token_dim and the class's own fields (tensors or numbers)."""
        with open(p, "wb") as f:
            np.savez(f, magic=np.array(magic), format=np.array(fmt), token_dim=np.array(self.token_dim),
                     **{k: v.cpu().numpy() if torch.is_tensor(v) else np.array(v) for k, v in fields.items()})

    def _read_archive(self, p: str, what: str, magic: str, fmt: int, width_of: str, rebuild_with: Optional[str] = None):
        """The archive at p after the checks every class makes: a zip at all (rebuild_with: the class tells a faiss file
        apart with a message of its own), this class's magic and format, the config's token_dim and the padded width of
        field `width_of`.  `what` = the class name with its article."""
        with open(p, "rb") as f:
            is_zip = f.read(4)[:2] == b"PK"
        if not is_zip and rebuild_with is not None:
            raise ops.NativeError(f"{p} is not {what} file (an index written by faiss cannot be read: build the index again "
                                  f"with {rebuild_with})")
        z = np.load(p, allow_pickle=False) if is_zip else None
        if z is None or "magic" not in z.files or str(z["magic"]) != magic or int(z["format"]) != fmt:
            raise ops.NativeError(f"{p} is not {what} file of format {fmt}")
        if int(z["token_dim"]) != self.token_dim or z[width_of].shape[1] != self.E_pad:
            raise ops.NativeError(f"{p} holds {int(z['token_dim'])}-dim vectors, the config says {self.token_dim}")
        return z


class FlatIPIndexer(_ShardedIndex):
    def __init__(self, config, device=None, group=None, topk_fn=None, merge_fn=None, merge_single_rank: bool = False):
        """topk_fn(queries, vectors, k) / merge_fn(scores, ids, k) default to the native operators
        (ops.dot_topk / ops.topk_merge); the CPU test-suite injects oracle stand-ins to exercise the
        sharding logic under gloo.  merge_single_rank: run the two all-gathers + the merge of the sharded search even
        when the process group has ONE rank (rehearsal of the multi-GPU path on a single-GPU box)."""
        self.merge_single_rank = bool(merge_single_rank)
        self._topk = topk_fn if topk_fn is not None else ops.dot_topk
        self._merge = merge_fn if merge_fn is not None else ops.topk_merge
        self._configure(config, device, group,
                        "FlatIPIndexer stores float16 vectors and rounds queries to float16 (faiss useFloat16 "
                        "semantics): set token_dtype: float16 (base_index.py:14), or keep faiss for an fp32 index")
        self.vectors: Optional[torch.Tensor] = None           # [n_local, E_pad]
        self.ids: Optional[torch.Tensor] = None               # [n_local] int64 external ids (IndexIDMap)

    def prepare(self, data_chunks: List[np.ndarray]):          # base_index.py: nothing to train for a flat index
        pass

    def index(self, ids: List[np.ndarray], data_chunks: List[np.ndarray]):
        """faiss_indices.py:22-27: one add of all vectors with their ids.  With several ranks each
        keeps its contiguous shard."""
        self.ids, self.vectors = self._shard(ids, data_chunks)

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        """This rank's shard handed over as device tensors (vectors [n_local, E_pad] float16, ids [n_local] int64) — for
        collections that are produced on the device (bench.py generates each rank's shard of the 8.8 M synthetic passages in
        place instead of materialising 13.6 GB of host arrays per rank)."""
        self._check_resident(ids, vectors)
        self.vectors, self.ids = vectors.contiguous(), ids.to(torch.int64).contiguous()

    def search_device(self, query_vec, top_n: int):
        """search() without the final copy to the host: device tensors (what a caller that keeps working on the GPU wants,
        and what bench.py times)."""
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        s, idx = self._topk(qd, self.vectors, top_n)
        return self._finish(s, self._ids_of(idx), top_n)


_IVF_MAGIC = "matchmaker_amd.IVFFlatIPIndexer"
_IVF_FORMAT = 1


class IVFFlatIPIndexer(_ShardedIndex):
    """Drop-in for the reference's GPU IVF index (`FaissIVFIndexer`, faiss_indices.py:106-145: inner-product inverted
    lists, fp16 scalar quantiser for centroids and lists, `co.shard` over the GPUs): `prepare(data_chunks, subsample)`
    trains `faiss_ivf_list_count` centroids by spherical k-means, `index(ids, data_chunks)` stores this rank's shard list
    by list, `search(query_vec, top_n)` probes the `faiss_ivf_search_probe_count` best lists of every query and returns
    the EXACT top_n of their union (ops.ivf_scan), merged over the ranks.  `save` / `load` use a file format of their own."""

    KMEANS_ITERS = 20            # faiss ClusteringParameters.niter
    ASSIGN_CHUNK = 1 << 14       # vectors per assignment call (bounds the top-k workspace)
    SUM_CHUNK = 1 << 18          # vectors per fp32 conversion of the centroid update

    def __init__(self, config, device=None, group=None, topk_fn=None, scan_fn=None, merge_fn=None, native_kmeans: bool = False,
                 assign_fn=None, sum_fn=None):
        """topk_fn(queries, vectors, k) / scan_fn(queries, vectors, list_begin, probes, k) / merge_fn(scores, ids, k)
        default to ops.dot_topk / ops.ivf_scan / ops.topk_merge; the CPU test-suite injects stand-ins.
        native_kmeans (opt-in): training and list assignment go through `spherical_kmeans` = ops.kmeans_assign /
        ops.kmeans_segment_sum (assign_fn / sum_fn stand in for them) instead of the top-k operator and index_add_: same
        sample, same loop, and centroids that are bit-equal from run to run."""
        self.native_kmeans = bool(native_kmeans)
        self._kassign = assign_fn if assign_fn is not None else ops.kmeans_assign
        self._ksum = sum_fn if sum_fn is not None else ops.kmeans_segment_sum
        self._topk = topk_fn if topk_fn is not None else ops.dot_topk
        self._scan = scan_fn if scan_fn is not None else ops.ivf_scan
        self._merge = merge_fn if merge_fn is not None else ops.topk_merge
        self._configure(config, device, group,
                        "IVFFlatIPIndexer stores float16 centroids and lists and rounds queries to float16 (the "
                        "reference's fp16 IVF: an fp16 scalar quantiser): set token_dtype: float16, or keep faiss "
                        "for an fp32 index")
        self.nlist = int(config["faiss_ivf_list_count"])
        self.nprobe = int(config["faiss_ivf_search_probe_count"])
        if self.nlist < 1 or self.nprobe < 1:
            raise ops.NativeError("faiss_ivf_list_count and faiss_ivf_search_probe_count must be positive")
        self.seed = int(config.get("random_seed", 208973249))
        self.centroids: Optional[torch.Tensor] = None         # [nlist, E_pad] unit length, float16
        self.vectors: Optional[torch.Tensor] = None           # [n_local, E_pad] list by list
        self.ids: Optional[torch.Tensor] = None               # [n_local] int64 external ids, same order
        self.list_begin: Optional[torch.Tensor] = None        # [nlist + 1] int64

    def _assign(self, x: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        """[n] int64: the centroid of maximum inner product for every row of x."""
        if self.native_kmeans:
            return self._kassign(x, centroids)[0].to(torch.int64)
        return _assign_by_topk(self._topk, x, centroids, self.ASSIGN_CHUNK, torch.int64)

    def _train_rows(self, n: int, subsample, gen) -> Optional[torch.Tensor]:
        """The seeded, sorted rows a subsample in (0, 1) trains on (host int64), or None for all of them."""
        if not 0 < subsample < 1:
            return None
        return torch.randperm(n, generator=gen)[: max(1, int(n * subsample))].sort().values

    def _check_train_size(self, n: int):
        if n < self.nlist:
            raise ops.NativeError(f"IVFFlatIPIndexer.prepare: {n} training vectors for faiss_ivf_list_count = {self.nlist}")

    def prepare(self, data_chunks: List[np.ndarray], subsample=-1):
        """Spherical k-means (faiss sets `spherical` for inner-product IVF), KMEANS_ITERS iterations from a seeded sample
        of the training vectors; subsample in (0, 1] trains on a seeded fraction of them: the rows are chosen on the host
        and only they are copied to the device.  An empty cluster is re-seeded from a vector of the largest cluster.
        Under torch.distributed rank 0 trains and its centroids are broadcast."""
        n_all = sum(c.shape[0] for c in data_chunks)
        gen = torch.Generator().manual_seed(self.seed)
        keep = self._train_rows(n_all, subsample, gen)
        self._check_train_size(n_all if keep is None else keep.numel())     # on every rank, before any collective
        x = None
        if self._world()[1] == 0:
            if keep is None:
                x = self._to_device(data_chunks, 0, n_all)
            else:
                k, off, parts = keep.numpy(), 0, []
                for c in data_chunks:
                    a, b = np.searchsorted(k, [off, off + c.shape[0]])
                    parts.append(np.ascontiguousarray(c[k[a:b] - off]))
                    off += c.shape[0]
                x = self._to_device(parts, 0, k.shape[0])
        self._train(x, gen)

    def train_resident(self, x: torch.Tensor, subsample=-1):
        """prepare() on training vectors that already are a device tensor [n, E_pad] float16."""
        gen = torch.Generator().manual_seed(self.seed)
        keep = self._train_rows(x.shape[0], subsample, gen)
        self._check_train_size(x.shape[0] if keep is None else keep.numel())
        self._train(x if keep is None else x[keep.to(x.device)], gen)

    def _train(self, x: Optional[torch.Tensor], gen):
        """k-means on rank 0 (x is None elsewhere), then the broadcast."""
        if self._world()[1] == 0:
            n = x.shape[0]
            cent = _unit_rows(x[torch.randperm(n, generator=gen)[: self.nlist].to(x.device)].float()).to(self.dtype)
            if self.native_kmeans:
                cent = spherical_kmeans(x, self.nlist, iters=self.KMEANS_ITERS, init=cent, assign_fn=self._kassign,
                                        sum_fn=self._ksum)
            for _ in range(0 if self.native_kmeans else self.KMEANS_ITERS):
                a = self._assign(x, cent)
                sums = torch.zeros((self.nlist, self.E_pad), dtype=torch.float32, device=x.device)
                for lo in range(0, n, self.SUM_CHUNK):      # fp32 copies of SUM_CHUNK rows at a time, in input order
                    sums.index_add_(0, a[lo: lo + self.SUM_CHUNK], x[lo: lo + self.SUM_CHUNK].float())
                counts = torch.bincount(a, minlength=self.nlist)
                empty = torch.nonzero(counts == 0).flatten()
                if empty.numel():
                    members = torch.nonzero(a == counts.argmax()).flatten()
                    sums[empty] = x[members[torch.arange(empty.numel(), device=x.device) % members.numel()]].float()
                cent = _unit_rows(sums).to(self.dtype)
        else:
            cent = torch.empty((self.nlist, self.E_pad), dtype=self.dtype, device=self.device)
        self._broadcast(cent)
        self.centroids = cent.contiguous()

    def index(self, ids: List[np.ndarray], data_chunks: List[np.ndarray]):
        """Every vector of this rank's contiguous shard goes to the list of its maximum-inner-product centroid; the shard
        is then stored list by list (stable: input order inside a list)."""
        if self.centroids is None:
            raise ops.NativeError("IVFFlatIPIndexer.index: prepare() (or load()) first")
        self.index_resident(*self._shard(ids, data_chunks))

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        """This rank's shard handed over as device tensors (vectors [n_local, E_pad] float16, ids [n_local] int64)."""
        self._check_resident(ids, vectors)
        order, self.list_begin, _ = _lists_of(self._assign(vectors, self.centroids), self.nlist)
        self.vectors = vectors[order].contiguous()
        self.ids = ids.to(torch.int64)[order].contiguous()

    def search_device(self, query_vec, top_n: int, return_probes: bool = False):
        """search() on device tensors; -inf / -1 where the probed lists ran out."""
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        probes = self._topk(qd, self.centroids, min(self.nprobe, self.nlist))[1].to(torch.int32)
        s, rows = self._scan(qd, self.vectors, self.list_begin, probes, top_n)
        s, ids = self._finish(s, self._ids_of(rows), top_n)
        return (s, ids, probes) if return_probes else (s, ids)

    def save(self, path: str):
        """One numpy .npz archive (this rank's shard; `path + ".rank<r>"` with several ranks)."""
        self._write_archive(self._rank_path(path), _IVF_MAGIC, _IVF_FORMAT, nprobe=self.nprobe, centroids=self.centroids,
                            list_begin=self.list_begin, vectors=self.vectors, ids=self.ids)

    def load(self, path: str, config_overwrites=None):
        """faiss_indices.py:143-145: the probe count comes from config_overwrites["faiss_ivf_search_probe_count"]."""
        _refuse_other_ivf_archive(self._rank_path(path), _IVF_FP8_MAGIC, "an IVFFlatIPIndexer", "IVFFp8IPIndexer")
        z = self._read_archive(self._rank_path(path), "an IVFFlatIPIndexer", _IVF_MAGIC, _IVF_FORMAT, "centroids",
                               rebuild_with="prepare() / index()")
        self.centroids = torch.from_numpy(z["centroids"]).to(self.device)
        self.list_begin = torch.from_numpy(z["list_begin"]).to(self.device)
        self.vectors = torch.from_numpy(z["vectors"]).to(self.device)
        self.ids = torch.from_numpy(z["ids"]).to(self.device)
        self.nlist = self.centroids.shape[0]
        self.nprobe = int(z["nprobe"])
        if config_overwrites is not None and "faiss_ivf_search_probe_count" in config_overwrites:
            self.nprobe = int(config_overwrites["faiss_ivf_search_probe_count"])


_IVF_FP8_MAGIC = "matchmaker_amd.IVFFp8IPIndexer"
_IVF_FP8_FORMAT = 1


class IVFFp8IPIndexer(IVFFlatIPIndexer):
    """IVFFlatIPIndexer whose lists hold the fp8 token store's rows: `codes` [n, E_pad] uint8 (OCP e4m3fn) +
    `scales` [n] float32 (one power of two per row) list by list, with `ids` and `list_begin` as before — half the bytes of
    the 16-bit lists, and no 16-bit copy of the rows.  Training, the centroid table (16-bit), the probe selection, the
    sharding and the merge are inherited; the probed lists are scanned by ops.ivf_scan_fp8 (the EXACT top_n of
    scale * <query, deq(code)> over their union).

    One assignment rule: a row goes to the list of the maximum-inner-product centroid of the value the index STORES,
    deq(code) * scale as float16 — whether it arrives as 16-bit vectors (index / index_resident: quantised first) or as
    codes + scales (index_codes), so the two build bit-equal indices.  `save` / `load` use an archive of their own."""

    DEQ_CHUNK = 1 << 20          # rows dequantised to float16 at a time (assignment, training sample)

    def __init__(self, config, device=None, group=None, topk_fn=None, scan_fn=None, merge_fn=None, native_kmeans: bool = False,
                 assign_fn=None, sum_fn=None, quantize_fn=None):
        """As IVFFlatIPIndexer, with scan_fn(queries, codes, scales, list_begin, probes, k) defaulting to ops.ivf_scan_fp8
        and quantize_fn(x) -> (codes, scales) to ops.fp8_quantize_rows."""
        super().__init__(config, device=device, group=group, topk_fn=topk_fn,
                         scan_fn=scan_fn if scan_fn is not None else ops.ivf_scan_fp8, merge_fn=merge_fn,
                         native_kmeans=native_kmeans, assign_fn=assign_fn, sum_fn=sum_fn)
        self._quantize = quantize_fn if quantize_fn is not None else ops.fp8_quantize_rows
        self.codes: Optional[torch.Tensor] = None             # [n_local, E_pad] uint8 list by list
        self.scales: Optional[torch.Tensor] = None            # [n_local] float32, same order

    @property
    def vectors(self):
        raise ops.NativeError("IVFFp8IPIndexer.vectors: the lists hold no 16-bit rows — read .codes / .scales "
                              "(ops.fp8_dequantize_rows gives their values)")

    @vectors.setter
    def vectors(self, value):                                 # the base constructor's `self.vectors = None` lands here
        if value is not None:
            raise ops.NativeError("IVFFp8IPIndexer.vectors: the lists hold no 16-bit rows — fill the index with "
                                  "index_resident() / index_codes(), which set .codes / .scales")

    def _check_codes(self, what: str, codes: torch.Tensor, scales: torch.Tensor):
        if (codes.dim() != 2 or codes.dtype != torch.uint8 or codes.shape[1] != self.E_pad or scales.dtype != torch.float32
                or tuple(scales.shape) != (codes.shape[0],)):
            raise ops.NativeError(f"IVFFp8IPIndexer.{what}: need uint8 [n, {self.E_pad}] codes and float32 [n] scales, got "
                                  f"{codes.dtype} {tuple(codes.shape)} / {scales.dtype} {tuple(scales.shape)}")

    def train_codes(self, codes: torch.Tensor, scales: torch.Tensor, subsample=-1):
        """train_resident() on rows that arrive as an fp8 store: the seeded sample (all rows without a subsample in (0, 1))
        dequantised to float16."""
        self._check_codes("train_codes", codes, scales)
        gen = torch.Generator().manual_seed(self.seed)
        keep = self._train_rows(codes.shape[0], subsample, gen)
        self._check_train_size(codes.shape[0] if keep is None else keep.numel())
        if keep is not None:
            keep = keep.to(codes.device)
            codes, scales = codes[keep], scales[keep]
        x = torch.cat([ops.fp8_dequantize_rows(codes[a: a + self.DEQ_CHUNK], scales[a: a + self.DEQ_CHUNK], self.dtype)
                       for a in range(0, max(codes.shape[0], 1), self.DEQ_CHUNK)])
        self._train(x, gen)

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        """This rank's shard as device tensors (vectors [n_local, E_pad] float16, ids [n_local] int64): quantised, then
        index_codes."""
        self._check_resident(ids, vectors)
        self.index_codes(ids, *self._quantize(vectors.contiguous()))

    def index_codes(self, ids: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor):
        """This rank's shard as an fp8 store (codes [n_local, E_pad] uint8, scales [n_local] float32, ids [n_local] int64):
        every row goes to the list of the best centroid of deq(code) * scale as float16, DEQ_CHUNK rows at a time; the shard
        is then stored list by list (stable: input order inside a list)."""
        if self.centroids is None:
            raise ops.NativeError("IVFFp8IPIndexer.index_codes: prepare() / train_codes() (or load()) first")
        self._check_codes("index_codes", codes, scales)
        if ids.shape[0] != codes.shape[0]:
            raise ops.NativeError(f"IVFFp8IPIndexer.index_codes: {ids.shape[0]} ids for {codes.shape[0]} rows")
        a = torch.empty(codes.shape[0], dtype=torch.int64, device=codes.device)
        for lo in range(0, codes.shape[0], self.DEQ_CHUNK):
            x = ops.fp8_dequantize_rows(codes[lo: lo + self.DEQ_CHUNK], scales[lo: lo + self.DEQ_CHUNK], self.dtype)
            a[lo: lo + self.DEQ_CHUNK] = self._assign(x.contiguous(), self.centroids)
        order, self.list_begin, _ = _lists_of(a, self.nlist)
        self.codes = codes[order].contiguous()
        self.scales = scales[order].contiguous()
        self.ids = ids.to(torch.int64)[order].contiguous()

    def search_device(self, query_vec, top_n: int, return_probes: bool = False):
        """search() on device tensors; -inf / -1 where the probed lists ran out."""
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        probes = self._topk(qd, self.centroids, min(self.nprobe, self.nlist))[1].to(torch.int32)
        s, rows = self._scan(qd, self.codes, self.scales, self.list_begin, probes, top_n)
        s, ids = self._finish(s, self._ids_of(rows), top_n)
        return (s, ids, probes) if return_probes else (s, ids)

    def save(self, path: str):
        """One numpy .npz archive (this rank's shard; `path + ".rank<r>"` with several ranks)."""
        self._write_archive(self._rank_path(path), _IVF_FP8_MAGIC, _IVF_FP8_FORMAT, nprobe=self.nprobe, centroids=self.centroids,
                            list_begin=self.list_begin, codes=self.codes, scales=self.scales, ids=self.ids)

    def load(self, path: str, config_overwrites=None):
        """As IVFFlatIPIndexer.load: the probe count comes from config_overwrites["faiss_ivf_search_probe_count"]."""
        p = self._rank_path(path)
        _refuse_other_ivf_archive(p, _IVF_MAGIC, "an IVFFp8IPIndexer", "IVFFlatIPIndexer")
        z = self._read_archive(p, "an IVFFp8IPIndexer", _IVF_FP8_MAGIC, _IVF_FP8_FORMAT, "centroids",
                               rebuild_with="prepare() / index()")
        self.centroids = torch.from_numpy(z["centroids"]).to(self.device)
        self.list_begin = torch.from_numpy(z["list_begin"]).to(self.device)
        self.codes = torch.from_numpy(z["codes"]).to(self.device)
        self.scales = torch.from_numpy(z["scales"]).to(self.device)
        self.ids = torch.from_numpy(z["ids"]).to(self.device)
        self.nlist = self.centroids.shape[0]
        self.nprobe = int(z["nprobe"])
        if config_overwrites is not None and "faiss_ivf_search_probe_count" in config_overwrites:
            self.nprobe = int(config_overwrites["faiss_ivf_search_probe_count"])


def _refuse_other_ivf_archive(p: str, other_magic: str, what: str, other_class: str):
    """The two IVF classes share a surface, not a file: an archive of the other one is refused by its writer's name."""
    with open(p, "rb") as f:
        if f.read(2) != b"PK":
            return
    z = np.load(p, allow_pickle=False)
    if "magic" in z.files and str(z["magic"]) == other_magic:
        raise ops.NativeError(f"{p} is not {what} file: it was written by {other_class} (load it with that class, or build "
                              "the index again)")


class DynamicIVFIndexer(_DeviceIndex):
    """Drop-in for the reference's dynamic IVF index (`FaissDynamicIndexer`, faiss_indices.py:307-428), the index behind
    TAS-Balanced query clustering (matchmaker/distillation/query_clusterer.py:187-221): `prepare` trains
    `faiss_ivf_list_count` centroids by spherical k-means (mm_kmeans_assign / mm_kmeans_segment_sum), `index_all` and
    `update` put every vector into the list of its maximum-inner-product centroid (`list_n_probe` = 1),
    `search_single` returns the exact top_n of the query's list together with the centroid it hit.  Single process, as
    the reference's.

    Storage: vectors, ids and list numbers are kept in ARRIVAL order on the device; the list-by-list view that the scan
    needs (`vectors`, `ids`, `list_begin`) is rebuilt by a stable sort the first time it is read after `index_all` /
    `update`.  That makes an update O(n), which is right for the clusterer's sizes (hundreds of thousands of queries,
    updated a batch at a time), not for a collection of billions.  Order inside a list (faiss promises none): arrival
    order; an updated entry moves to the end of its new list.

    Differences from the reference: centroids and vectors are float16 (faiss keeps fp32 centroids beside its fp16
    lists) and queries are rounded to float16; `prepare(subsample >= 0)` trains on the sampled rows only, not on the zero
    rows the reference's integer division leaves at the end of its training matrix."""

    KMEANS_ITERS = 20            # faiss ClusteringParameters.niter

    def __init__(self, config, device=None, assign_fn=None, sum_fn=None, scan_fn=None):
        """assign_fn(x, centroids) / sum_fn(x, order, list_begin) / scan_fn(queries, vectors, list_begin, probes, k) default
        to ops.kmeans_assign / ops.kmeans_segment_sum / ops.ivf_scan; the CPU test-suite injects stand-ins."""
        self._kassign = assign_fn if assign_fn is not None else ops.kmeans_assign
        self._ksum = sum_fn if sum_fn is not None else ops.kmeans_segment_sum
        self._scan = scan_fn if scan_fn is not None else ops.ivf_scan
        self.list_n_probe = 1
        self.faiss_ivf_list_count = int(config["faiss_ivf_list_count"])
        self.nlist = self.faiss_ivf_list_count
        if not 1 <= self.nlist <= 65536:
            raise ops.NativeError("faiss_ivf_list_count must be in 1 .. 65536")
        self._configure(config, device, "DynamicIVFIndexer stores float16 centroids and lists and rounds queries to float16: "
                        "set token_dtype: float16, or keep faiss for an fp32 index")
        self.seed = int(config.get("random_seed", 208973249))
        self.centroids: Optional[torch.Tensor] = None         # [nlist, E_pad] unit length, float16
        self._vec = torch.zeros((0, self.E_pad), dtype=self.dtype, device=self.device)      # arrival order
        self._ids = torch.zeros(0, dtype=torch.int64, device=self.device)
        self._lists = torch.zeros(0, dtype=torch.int64, device=self.device)
        self._view = None                                      # (vectors, ids, list_begin, ids on the host, list_begin on the host)

    # ---- training -----------------------------------------------------------------------------------------------------
    @staticmethod
    def train_rows(chunk_sizes: List[int], subsample) -> List[np.ndarray]:
        """The rows of every chunk but the last that `prepare(subsample > -1)` trains on: faiss_indices.py:335-345 —
        RandomState(123), one choice(..., replace=False) of int(total * subsample) // (len(chunks) - 1) rows per chunk, in
        chunk order."""
        if len(chunk_sizes) < 2:
            raise ops.NativeError("DynamicIVFIndexer.prepare: subsample needs at least two chunks (rows are drawn from every "
                                  "chunk but the last; the reference divides by len(data_chunks) - 1 = 0 here)")
        per_chunk = int(sum(chunk_sizes) * subsample) // (len(chunk_sizes) - 1)
        rs = np.random.RandomState(123)
        return [rs.choice(c, size=per_chunk, replace=False) for c in chunk_sizes[:-1]]

    def prepare(self, data_chunks: List[np.ndarray], subsample=-1):
        """subsample = -1 trains on every vector; subsample > -1 on the rows `train_rows` names."""
        if subsample > -1:
            rows = self.train_rows([c.shape[0] for c in data_chunks], subsample)
            parts = [c[r] for c, r in zip(data_chunks, rows)]
        else:
            parts = list(data_chunks)
        n = sum(p.shape[0] for p in parts)
        if n < self.nlist:
            raise ops.NativeError(f"DynamicIVFIndexer.prepare: {n} training vectors for faiss_ivf_list_count = {self.nlist}")
        x = self._to_device(parts, 0, n)
        self.centroids = spherical_kmeans(x, self.nlist, iters=self.KMEANS_ITERS, seed=self.seed, assign_fn=self._kassign,
                                          sum_fn=self._ksum)

    # ---- entries ------------------------------------------------------------------------------------------------------
    def _add(self, ids: np.ndarray, data: np.ndarray):
        if self.centroids is None:
            raise ops.NativeError("DynamicIVFIndexer: prepare() first")
        if data.shape[0] != ids.shape[0]:
            raise ops.NativeError(f"DynamicIVFIndexer: {ids.shape[0]} ids for {data.shape[0]} vectors")
        if ids.shape[0] == 0:
            return
        vec = self._to_device([data], 0, data.shape[0])
        self._vec = torch.cat([self._vec, vec])
        self._ids = torch.cat([self._ids, torch.from_numpy(ids).to(self.device)])
        self._lists = torch.cat([self._lists, self._kassign(vec, self.centroids)[0].to(torch.int64)])
        self._view = None

    def index_all(self, ids, data_chunks):
        """faiss_indices.py:355-359: chunk i adds its first len(ids[i]) vectors under ids[i]."""
        i = [np.array(x, dtype=np.int64) for x in ids]
        self._add(np.concatenate(i) if i else np.zeros(0, np.int64),
                  np.concatenate([np.asarray(c)[: len(k)] for c, k in zip(data_chunks, i)]) if i else np.zeros((0, self.token_dim)))

    def update(self, ids, data):
        """faiss_indices.py:368-375: every stored entry whose id is in `ids` is removed, then data[:len(ids)] is added under
        those ids, assigned to the unchanged centroids (unknown ids are simply added)."""
        ids = np.array(ids, dtype=np.int64)
        keep = ~torch.isin(self._ids, torch.from_numpy(ids).to(self.device))
        self._vec, self._ids, self._lists = self._vec[keep], self._ids[keep], self._lists[keep]
        self._view = None
        self._add(ids, np.asarray(data)[: len(ids)])

    def _lists_view(self):
        if self._view is None:
            order, lb, _ = _lists_of(self._lists, self.nlist)
            ids = self._ids[order].contiguous()
            self._view = (self._vec[order].contiguous(), ids, lb, ids.cpu().numpy(), lb.cpu().numpy())
        return self._view

    @property
    def vectors(self) -> torch.Tensor:
        """[n, E_pad] float16, list by list"""
        return self._lists_view()[0]

    @property
    def ids(self) -> torch.Tensor:
        """[n] int64 external ids, in the order of `vectors`"""
        return self._lists_view()[1]

    @property
    def list_begin(self) -> torch.Tensor:
        """[nlist + 1] int64"""
        return self._lists_view()[2]

    def get_entries_from_centroids(self, centroid_ids) -> list:
        """faiss_indices.py:383-393: the ids stored in the named lists, list after list (arrival order inside a list)."""
        _, _, _, ids, lb = self._lists_view()
        out = []
        for l in centroid_ids:
            out.extend(ids[lb[int(l)]: lb[int(l) + 1]].tolist())
        return out

    def get_all_cluster_assignments(self) -> list:
        return [self.get_entries_from_centroids([c]) for c in range(self.nlist)]

    # ---- search -------------------------------------------------------------------------------------------------------
    def assign(self, query_vecs) -> torch.Tensor:
        """[nq] int64 (device): the centroid of maximum inner product of every query (lowest number on equal scores)."""
        if self.centroids is None:
            raise ops.NativeError("DynamicIVFIndexer: prepare() first")
        qd = _device_queries(query_vecs, self.dtype, self.E_pad, self.token_dim, self.device)
        return self._kassign(qd, self.centroids)[0].to(torch.int64)

    def cluster_assignments(self, query_vecs, seq_ids) -> List[list]:
        """The loop of query_clusterer.py:205-221 as one device call: clusters[c] = the seq_ids whose query hits centroid c,
        in input order."""
        a = self.assign(query_vecs).cpu().tolist()
        if len(a) != len(seq_ids):
            raise ops.NativeError(f"cluster_assignments: {len(seq_ids)} seq_ids for {len(a)} queries")
        clusters = [[] for _ in range(self.nlist)]
        for c, sid in zip(a, seq_ids):
            clusters[c].append(sid)
        return clusters

    def search_single(self, query_vec, top_n: int):
        """faiss_indices.py:401-428: (scores [nq, top_n] float32 descending, ids [nq, top_n] int64, centroid_ids [nq, 1]
        int64) as numpy arrays; (-inf, -1) where the list holds fewer than top_n entries."""
        if self.centroids is None:
            raise ops.NativeError("DynamicIVFIndexer: prepare() first")
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        cids = self._kassign(qd, self.centroids)[0]
        s, rows = self._scan(qd, self.vectors, self.list_begin, cids.to(torch.int32)[:, None].contiguous(), top_n)
        return s.cpu().numpy(), self._ids_of(rows).cpu().numpy(), cids.to(torch.int64)[:, None].cpu().numpy()


_GRAPH_MAGIC = "matchmaker_amd.GraphIPIndexer"
_GRAPH_FORMAT = 1


_KNN_EXACT_ROWS = 16          # query rows per sorted fallback of _knn_block


def _knn_block(vectors: torch.Tensor, lo: int, hi: int, k: int, topk_fn) -> torch.Tensor:
    """[hi - lo, k] int64: topk_fn(vectors[lo:hi], vectors, k)[1].  ops.dot_topk thresholds every query from a sample of the
    shard and gives up on a query it cannot decide in its re-runs (met on a clustered 1.1 M x 768 shard searched against
    itself: 6 rows of 1.1 M); it then raises for the whole call.  The block is halved until the undecided rows are isolated
    in pieces of at most _KNN_EXACT_ROWS rows, and those are ranked in full: fp32 inner products of the stored 16-bit rows
    with the whole shard, stable sort = score descending, lower row first — the same rule, without a threshold."""
    try:
        return topk_fn(vectors[lo:hi], vectors, k)[1]
    except ops.NativeError:
        if hi - lo > _KNN_EXACT_ROWS:
            mid = (lo + hi) // 2
            return torch.cat([_knn_block(vectors, lo, mid, k, topk_fn), _knn_block(vectors, mid, hi, k, topk_fn)])
    N = vectors.shape[0]
    q = vectors[lo:hi].float()
    scores = torch.empty((hi - lo, N), dtype=torch.float32, device=vectors.device)
    for a in range(0, N, 1 << 18):
        scores[:, a: a + (1 << 18)] = q @ vectors[a: a + (1 << 18)].float().t()
    idx = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
    if idx.shape[1] < k:
        idx = torch.nn.functional.pad(idx, (0, k - idx.shape[1]), value=-1)
    return idx


def build_graph(vectors: torch.Tensor, M: int, topk_fn=None, block: int = 1 << 14) -> torch.Tensor:
    """The neighbour graph of a shard: vectors [N, E_pad] float16 / bfloat16 -> neighbors [N, M] int32, -1 padded.

    1. knn[v] = the M rows of highest inner product with row v without v itself, score descending, lower row first on
       ties: topk_fn(k = M + 1) over the stored vectors in query blocks (rows the top-k operator cannot decide are ranked
       in full, `_knn_block`); v is dropped from its own list when present, otherwise the last entry is; -1 padded when
       N - 1 < M.
    2. forward edges fwd[v] = knn[v][:M/2].
    3. reverse edges: v receives u for every edge u -> v of fwd, ordered by (rank of v in fwd[u], u), skipping any u
       already in the row, until the row holds M entries.
    4. fill: knn[v][M/2:] in order, skipping entries already present, until the row holds M entries.
    Steps 2-4 are sorted torch ops on the vectors' device: the three sources are laid out in priority order, one stable
    sort by destination row gives every row its sequence, a second stable sort by (row, value) finds repeats."""
    topk_fn = topk_fn if topk_fn is not None else ops.dot_topk
    if M % 2 or not 2 <= M <= 128:
        raise ops.NativeError(f"faiss_hnsw_graph_neighbors = {M} must be an even number in 2 .. 128")
    N, dev = vectors.shape[0], vectors.device
    if N >= 1 << 31:
        raise ops.NativeError("build_graph: more than 2^31-1 vectors in one shard")
    H = M // 2
    knn = torch.empty((N, M), dtype=torch.int64, device=dev)
    for lo in range(0, N, block):
        idx = _knn_block(vectors, lo, min(N, lo + block), M + 1, topk_fn)
        own = idx == torch.arange(lo, lo + idx.shape[0], device=dev)[:, None]
        own[:, -1] |= ~own.any(dim=1)
        knn[lo: lo + block] = idx[~own].view(-1, M)            # exactly one entry leaves every row, the order stays
    rows = torch.arange(N, device=dev)
    # (destination row, value) in priority order: forward edges by rank, reverse edges by (rank, source), fill by rank
    dest = torch.cat([rows.repeat(H), knn[:, :H].t().reshape(-1), rows.repeat(M - H)])
    val = torch.cat([knn[:, :H].t().reshape(-1), rows.repeat(H), knn[:, H:].t().reshape(-1)])
    ok = (dest >= 0) & (val >= 0)
    dest, val = dest[ok], val[ok]
    order = torch.sort(dest, stable=True).indices
    dest, val = dest[order], val[order]
    by_pair = torch.sort(dest * N + val, stable=True)
    first = torch.ones_like(dest, dtype=torch.bool)
    first[1:] = by_pair.values[1:] != by_pair.values[:-1]
    keep = torch.empty_like(first)
    keep[by_pair.indices] = first                                # the first occurrence of a value in its row stays
    dest, val = dest[keep], val[keep]
    begin = torch.searchsorted(dest, rows)
    rank = torch.arange(dest.shape[0], device=dev) - begin[dest]
    fits = rank < M
    out = torch.full((N, M), -1, dtype=torch.int32, device=dev)
    out[dest[fits], rank[fits]] = val[fits].to(torch.int32)
    return out


class GraphIPIndexer(_ShardedIndex):
    """Drop-in for the reference's HNSW index (`FaissHNSWIndexer`, faiss_indices.py: IndexHNSWFlat with
    `faiss_hnsw_graph_neighbors` links, `efSearch`, inner product; a CPU index there — "HNSW does not support GPUs"):
    `prepare` has nothing to train, `index(ids, data_chunks)` stores this rank's shard and builds its neighbour graph
    (`build_graph`), `search(query_vec, top_n)` picks `graph_entry_count` entry rows out of a strided sample of
    `graph_entry_sample` rows with the top-k kernel and runs the beam search (ops.graph_search) with
    ef = max(faiss_hnsw_efSearch, top_n), merged over the ranks.  `save` / `load` use a file format of their own.

    Differences from the reference: ONE level, no hierarchy; the construction is exact (no incremental insertion), so
    `faiss_hnsw_efConstruction` is accepted and ignored; vectors are float16 and queries are rounded to float16; equal
    scores come lower row first.  Recall figures are this graph's, not HNSW's."""

    def __init__(self, config, device=None, group=None, topk_fn=None, search_fn=None, merge_fn=None):
        """topk_fn(queries, vectors, k) / search_fn(queries, vectors, neighbors, entry_rows, ef, k, width) /
        merge_fn(scores, ids, k) default to ops.dot_topk / ops.graph_search / ops.topk_merge; the CPU test-suite injects
        stand-ins."""
        self._topk = topk_fn if topk_fn is not None else ops.dot_topk
        self._search = search_fn if search_fn is not None else ops.graph_search
        self._merge = merge_fn if merge_fn is not None else ops.topk_merge
        self._configure(config, device, group, "GraphIPIndexer stores float16 vectors and rounds queries to float16: set "
                        "token_dtype: float16, or keep faiss for an fp32 index")
        self.M = int(config["faiss_hnsw_graph_neighbors"])
        self.ef_search = int(config["faiss_hnsw_efSearch"])
        self.ef_construction = config.get("faiss_hnsw_efConstruction")       # accepted, ignored: the construction is exact
        self.entry_sample = int(config.get("graph_entry_sample", 4096))
        self.entry_count = int(config.get("graph_entry_count", 32))
        self.width = int(config.get("graph_search_width", 4))
        if self.M % 2 or not 2 <= self.M <= 128:
            raise ops.NativeError(f"faiss_hnsw_graph_neighbors = {self.M} must be an even number in 2 .. 128")
        if self.ef_search < 1 or self.entry_sample < 1 or self.entry_count < 1 or not 1 <= self.width <= 8:
            raise ops.NativeError("faiss_hnsw_efSearch, graph_entry_sample and graph_entry_count must be positive, "
                                  "graph_search_width in 1 .. 8")
        self.vectors: Optional[torch.Tensor] = None           # [n_local, E_pad]
        self.ids: Optional[torch.Tensor] = None               # [n_local] int64 external ids
        self.neighbors: Optional[torch.Tensor] = None         # [n_local, M] int32, -1 padded
        self.sample_rows: Optional[torch.Tensor] = None       # [S] int64 rows of the entry sample
        self.sample_vectors: Optional[torch.Tensor] = None    # [S, E_pad] their vectors, contiguous

    def prepare(self, data_chunks: List[np.ndarray] = None, subsample=-1):      # nothing to train
        pass

    def index(self, ids: List[np.ndarray], data_chunks: List[np.ndarray]):
        """This rank's contiguous shard of the vectors (every rank is given the same full lists) and its graph."""
        self.index_resident(*self._shard(ids, data_chunks))

    def _set_sample(self):
        n = self.vectors.shape[0]
        S = min(n, self.entry_sample)
        self.sample_rows = (torch.arange(S, dtype=torch.int64, device=self.vectors.device) * n) // max(S, 1)
        self.sample_vectors = self.vectors[self.sample_rows].contiguous()

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        """This rank's shard handed over as device tensors (vectors [n_local, E_pad] float16, ids [n_local] int64)."""
        self._check_resident(ids, vectors)
        self.vectors, self.ids = vectors.contiguous(), ids.to(torch.int64).contiguous()
        self.neighbors = build_graph(self.vectors, self.M, self._topk)
        self._set_sample()

    def entry_rows(self, qd: torch.Tensor, ef: int) -> torch.Tensor:
        """[nq, min(graph_entry_count, ef, S)] int32: the rows of the sample with the highest inner product."""
        S = self.sample_rows.shape[0]
        i = self._topk(qd, self.sample_vectors, min(self.entry_count, ef, S))[1]
        return torch.where(i >= 0, self.sample_rows[i.clamp(min=0)], i).to(torch.int32)

    def search_device(self, query_vec, top_n: int, return_rows: bool = False):
        """search() on device tensors; -inf / -1 where the search reached fewer rows."""
        if self.neighbors is None:
            raise ops.NativeError("GraphIPIndexer.search: index() (or load()) first")
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        ef = max(self.ef_search, int(top_n))                      # as faiss: efSearch never below k
        if self.vectors.shape[0] == 0:
            s = torch.full((qd.shape[0], top_n), float("-inf"), dtype=torch.float32, device=qd.device)
            rows = torch.full((qd.shape[0], top_n), -1, dtype=torch.int64, device=qd.device)
        else:
            s, rows = self._search(qd, self.vectors, self.neighbors, self.entry_rows(qd, ef), ef, top_n, self.width)
        s, ids = self._finish(s, self._ids_of(rows), top_n)
        return (s, ids, rows) if return_rows else (s, ids)

    def save(self, path: str):
        """One numpy .npz archive (this rank's shard; `path + ".rank<r>"` with several ranks)."""
        self._write_archive(self._rank_path(path), _GRAPH_MAGIC, _GRAPH_FORMAT, M=self.M, vectors=self.vectors, ids=self.ids,
                            neighbors=self.neighbors, sample_rows=self.sample_rows)

    def load(self, path: str, config_overwrites=None):
        """The file decides what was built (vectors, ids, graph, M, entry sample); the config decides how it is searched
        (efSearch, graph_entry_count, graph_search_width), and config_overwrites["faiss_hnsw_efSearch"] overrides efSearch."""
        p = self._rank_path(path)
        z = self._read_archive(p, "a GraphIPIndexer", _GRAPH_MAGIC, _GRAPH_FORMAT, "vectors", rebuild_with="index()")
        n, M = z["vectors"].shape[0], int(z["M"])
        nb, sr = z["neighbors"], z["sample_rows"]
        if (z["ids"].shape != (n,) or nb.shape != (n, M) or nb.dtype != np.int32 or z["vectors"].dtype != np.float16 or M % 2
                or not 2 <= M <= 128 or sr.ndim != 1 or (n > 0 and (sr.size == 0 or sr.min() < 0 or sr.max() >= n))
                or (nb.size and (nb.min() < -1 or nb.max() >= n))):
            raise ops.NativeError(f"{p} is damaged: vectors {z['vectors'].shape} {z['vectors'].dtype}, ids {z['ids'].shape}, "
                                  f"neighbors {nb.shape} {nb.dtype} for M = {M}, sample rows outside the shard or none")
        self.vectors = torch.from_numpy(z["vectors"]).to(self.device)
        self.ids = torch.from_numpy(z["ids"].astype(np.int64)).to(self.device)
        self.neighbors = torch.from_numpy(nb).to(self.device)
        self.sample_rows = torch.from_numpy(sr.astype(np.int64)).to(self.device)
        self.sample_vectors = self.vectors[self.sample_rows].contiguous()
        # the graph and its sample are what the file holds: M and the sample size come from the file; the search knobs
        # (efSearch, entry count, width) stay the config's
        self.M, self.entry_sample = M, int(sr.size)
        if config_overwrites is not None and "faiss_hnsw_efSearch" in config_overwrites:
            self.ef_search = int(config_overwrites["faiss_hnsw_efSearch"])


_SCANN_MAGIC = "matchmaker_amd.ScannIPIndexer"
_SCANN_FORMAT = 1
_SCANN_FILE = "scann_ip.npz"


def _segment_sum_torch(x: torch.Tensor, order: torch.Tensor, list_begin: torch.Tensor) -> torch.Tensor:
    """ops.kmeans_segment_sum in torch (host stand-in paths only)."""
    nlist = list_begin.shape[0] - 1
    lists = torch.repeat_interleave(torch.arange(nlist, device=x.device), torch.diff(list_begin))
    return torch.zeros((nlist, x.shape[1]), dtype=torch.float32, device=x.device).index_add_(0, lists, x[order].float())


def train_ah_codebook(residuals: torch.Tensor, iters: int = 10, seed: int = 208973249, chunk: int = 1 << 14) -> torch.Tensor:
    """The codebook of the 4-bit codes: residuals [m, E] float32 -> [E / 2, 16, 2] float32, 16 centres per 2-dimensional
    block by plain (Euclidean) k-means, `iters` iterations from 16 rows drawn with `seed` (the same rows for every block;
    repeated when m < 16).  Assignment = nearest centre, lowest number on equal distance; the update sums every centre's
    members with masked reductions over row chunks in a fixed order (no atomics, no scatter), so two runs from one seed
    give bit-equal codebooks; a centre without members keeps its place."""
    m, E = residuals.shape
    S = E // 2
    if m < 1:
        raise ops.NativeError("train_ah_codebook: no training rows")
    r = residuals.reshape(m, S, 2)
    gen = torch.Generator().manual_seed(int(seed))
    rows = torch.randperm(m, generator=gen)[:16]
    rows = rows[torch.arange(16) % rows.numel()].to(r.device)
    cb = r[rows].permute(1, 0, 2).contiguous()                     # [S, 16, 2]
    for _ in range(iters):
        sums = torch.zeros((S, 16, 2), dtype=torch.float32, device=r.device)
        counts = torch.zeros((S, 16), dtype=torch.float32, device=r.device)
        for lo in range(0, m, chunk):
            rc = r[lo: lo + chunk]                                 # [c, S, 2]
            d0 = rc[:, :, None, 0] - cb[None, :, :, 0]
            d1 = rc[:, :, None, 1] - cb[None, :, :, 1]
            a = torch.argmin(d0 * d0 + d1 * d1, dim=2)             # [c, S]
            for k in range(16):
                mk = (a == k).to(torch.float32)
                sums[:, k] += (rc * mk[:, :, None]).sum(dim=0)
                counts[:, k] += mk.sum(dim=0)
        cb = torch.where(counts[:, :, None] > 0, sums / counts[:, :, None].clamp_min(1.0), cb)
    return cb


class ScannIPIndexer(_ShardedIndex):
    """Drop-in for the reference's ScaNN index (`ScaNNIndexer`, matchmaker/retrieval/scann_index.py:10-53: scann's
    `.tree(num_leaves=int(sqrt(n)), num_leaves_to_search=100).score_ah(2, anisotropic_quantization_threshold=0.2)
    .reorder(top_n)`, a CPU library there).  `prepare` is a no-op, `index(ids, data_chunks)` trains the leaves (spherical
    k-means) and the codebook, stores this rank's shard leaf by leaf — 4-bit codes for the scan, the float16 originals
    for the re-score —, `search(query_vec, top_n)` probes min(100, leaves) leaves, takes the best max(top_n, reorder)
    rows by their quantized scores (ops.ah_scan), re-scores them exactly (ops.gather_dot) and returns the top_n, merged
    over the ranks.  `save(path)` / `load(path)` use a directory, as scann's serialize does, with a file format of their own.

    Config keys that are NOT the reference's (all optional): scann_num_leaves, scann_leaves_to_search, scann_reorder,
    scann_anisotropic_threshold.

    Differences from ScaNN (which cannot be installed here: parity is unpinned): the tree is our spherical k-means on a
    seeded sample of at most KMEANS_TRAIN_ROWS rows; the codebook is plain k-means over residual blocks
    (`train_ah_codebook`), not ScaNN's anisotropic codebook training; the encoder runs a fixed schedule (nearest codeword,
    then DESCENT_PASSES ascending sweeps of coordinate descent); eta is the closed form (token_dim - 1) T^2 / (1 - T^2);
    scores come from decoded codewords through MFMA, not from SIMD LUT16 look-up tables with quantized sums; vectors and
    queries are float16; equal scores come lower row first."""

    KMEANS_ITERS = 20
    KMEANS_TRAIN_ROWS = 1 << 18   # rows of the seeded sample the leaves are trained on
    CODEBOOK_ITERS = 10
    CODEBOOK_TRAIN_ROWS = 1 << 16
    DESCENT_PASSES = 2
    ASSIGN_CHUNK = 1 << 14

    def __init__(self, config, device=None, group=None, topk_fn=None, encode_fn=None, scan_fn=None, rescore_fn=None,
                 merge_fn=None):
        """topk_fn(queries, vectors, k) / encode_fn(x, lists, centroids, codebook, eta, passes) / scan_fn(queries, codes,
        codebook, list_begin, probes, probe_scores, k) / rescore_fn(queries, vectors, rows) / merge_fn(scores, ids, k)
        default to ops.dot_topk / ops.ah_encode / ops.ah_scan / ops.gather_dot / ops.topk_merge; the CPU test-suite injects
        stand-ins.  With the native top-k the leaves are trained by `spherical_kmeans` on ops.kmeans_assign /
        ops.kmeans_segment_sum; an injected topk_fn also stands in for the assignment."""
        self._native = topk_fn is None
        self._topk = topk_fn if topk_fn is not None else ops.dot_topk
        self._encode = encode_fn if encode_fn is not None else ops.ah_encode
        self._scan = scan_fn if scan_fn is not None else ops.ah_scan
        self._rescore = rescore_fn if rescore_fn is not None else ops.gather_dot
        self._merge = merge_fn if merge_fn is not None else ops.topk_merge
        # token_dtype alone decides here: `faiss_use_fp16`, the override the faiss-shaped indices honour, is not read
        self._configure(config, device, group,
                        "ScannIPIndexer stores float16 originals, float16 centres and a float16 codebook and rounds "
                        "queries to float16: set token_dtype: float16, or keep scann for an fp32 index", fp16_override=False)
        self.num_leaves = config.get("scann_num_leaves")                       # None: int(sqrt(n)) at index time
        self.leaves_to_search = int(config.get("scann_leaves_to_search", 100))
        self.threshold = float(config.get("scann_anisotropic_threshold", 0.2))
        if "scann_reorder" in config:
            self.reorder = int(config["scann_reorder"])
        elif config.get("query_sets"):
            c = next(iter(config["query_sets"].values()))                      # scann_index.py:21-22
            self.reorder = int(c.get("index_hit_top_n", c["top_n"]))
        else:
            raise ops.NativeError("ScannIPIndexer: the reorder count comes from the first entry of query_sets "
                                  "(index_hit_top_n, else top_n) or from scann_reorder: neither is configured")
        if (self.num_leaves is not None and int(self.num_leaves) < 1) or self.leaves_to_search < 1 or self.reorder < 1 \
                or not 0.0 <= self.threshold < 1.0:
            raise ops.NativeError("scann_num_leaves, scann_leaves_to_search and scann_reorder must be positive, "
                                  "scann_anisotropic_threshold in [0, 1)")
        T2 = self.threshold * self.threshold
        self.eta = (self.token_dim - 1) * T2 / (1.0 - T2) if self.threshold > 0 else 1.0
        self.seed = int(config.get("random_seed", 208973249))
        self.nlist: Optional[int] = None
        self.centroids: Optional[torch.Tensor] = None         # [nlist, E_pad] unit length, float16
        self.codebook: Optional[torch.Tensor] = None          # [E_pad / 2, 16, 2] float16
        self.codes: Optional[torch.Tensor] = None             # [n_local, E_pad / 4] uint8, leaf by leaf
        self.vectors: Optional[torch.Tensor] = None           # [n_local, E_pad] float16, same order
        self.ids: Optional[torch.Tensor] = None               # [n_local] int64 external ids, same order
        self.list_begin: Optional[torch.Tensor] = None        # [nlist + 1] int64

    def prepare(self, data_chunks: List[np.ndarray] = None, subsample=-1):      # scann trains inside index()
        pass

    def _assign(self, x: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
        """[n] int32: the centre of maximum inner product of every row (lowest number on equal scores)."""
        if self._native:
            return ops.kmeans_assign(x, centroids)[0]
        return _assign_by_topk(self._topk, x, centroids, self.ASSIGN_CHUNK, torch.int32)

    def _sample(self, x: torch.Tensor, rows: int, gen) -> torch.Tensor:
        if x.shape[0] <= rows:
            return x
        return x[torch.randperm(x.shape[0], generator=gen)[:rows].sort().values.to(x.device)]

    def _train(self, x: Optional[torch.Tensor], n_all: int):
        """Leaves and codebook on rank 0 (x: its training vectors; None elsewhere), then the broadcast."""
        nlist = int(self.num_leaves) if self.num_leaves is not None else max(1, int(np.sqrt(n_all)))
        if self._world()[1] == 0:
            if x.shape[0] < nlist:
                raise ops.NativeError(f"ScannIPIndexer.index: {x.shape[0]} training vectors for {nlist} leaves")
            gen = torch.Generator().manual_seed(self.seed)
            xs = self._sample(x, self.KMEANS_TRAIN_ROWS, gen)
            kw = {} if self._native else dict(assign_fn=lambda a, c: (self._assign(a, c), None), sum_fn=_segment_sum_torch)
            cent = spherical_kmeans(xs, nlist, iters=self.KMEANS_ITERS, seed=self.seed, **kw)
            xc = self._sample(xs, self.CODEBOOK_TRAIN_ROWS, gen)
            res = xc.float() - cent[self._assign(xc, cent).to(torch.int64)].float()
            cb = train_ah_codebook(res, self.CODEBOOK_ITERS, self.seed).to(self.dtype)
        else:
            cent = torch.empty((nlist, self.E_pad), dtype=self.dtype, device=self.device)
            cb = torch.empty((self.E_pad // 2, 16, 2), dtype=self.dtype, device=self.device)
        self._broadcast(cent, cb)
        self.nlist, self.centroids, self.codebook = nlist, cent.contiguous(), cb.contiguous()

    def index(self, ids: List[np.ndarray], data_chunks: List[np.ndarray]):
        """scann_index.py:24-35: trains on the whole collection (rank 0, broadcast), then every rank stores its contiguous
        shard leaf by leaf (stable: input order inside a leaf) as codes and originals."""
        i = np.concatenate(ids).astype(np.int64)
        n_all = i.shape[0]
        world, rank = self._world()
        lo, hi = shard_range(n_all, world, rank)
        x_all = self._to_device(data_chunks, 0, n_all) if rank == 0 else None
        self._train(x_all, n_all)
        mine = x_all[lo:hi] if rank == 0 else self._to_device(data_chunks, lo, hi)
        self._store(torch.from_numpy(i[lo:hi]).to(self.device), mine)

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        """This rank's shard handed over as device tensors (vectors [n_local, E_pad] float16, ids [n_local] int64); rank 0
        trains on its own shard, the leaf count comes from the size of all shards."""
        self._check_resident(ids, vectors)
        world, rank = self._world()
        n_all = torch.tensor([vectors.shape[0]], dtype=torch.int64, device=vectors.device)
        if world > 1:
            dist.all_reduce(n_all, group=self.group)
        self._train(vectors if rank == 0 else None, int(n_all))
        self._store(ids, vectors)

    def _store(self, ids: torch.Tensor, vectors: torch.Tensor):
        a = self._assign(vectors, self.centroids)
        order, lb, _ = _lists_of(a, self.nlist)
        self.vectors = vectors[order].contiguous()
        self.ids = ids.to(torch.int64)[order].contiguous()
        self.list_begin = lb
        self.codes = self._encode(self.vectors, a[order].to(torch.int32).contiguous(), self.centroids, self.codebook,
                                  self.eta, self.DESCENT_PASSES)

    def search_device(self, query_vec, top_n: int, return_stages: bool = False):
        """scann_index.py:37-47 on device tensors: the scores are exact inner products; -inf / -1 where the probed leaves ran
        out.  return_stages: also (probes, quantized scores, candidate rows, exact scores)."""
        if self.codes is None:
            raise ops.NativeError("ScannIPIndexer.search: index() (or load()) first")
        top_n = int(top_n)
        if not 1 <= top_n <= 4096:
            raise ops.NativeError(f"ScannIPIndexer.search: top_n = {top_n} outside 1 .. 4096")
        qd = _device_queries(query_vec, self.dtype, self.E_pad, self.token_dim, self.device)
        ps, probes = self._topk(qd, self.centroids, min(self.leaves_to_search, self.nlist))
        probes = probes.to(torch.int32)
        k = min(max(top_n, self.reorder), 4096)
        qs, rows = self._scan(qd, self.codes, self.codebook, self.list_begin, probes, ps.to(torch.float32), k)
        exact = self._rescore(qd, self.vectors, rows)
        s, best = self._merge(exact, rows, top_n)                  # equal exact scores keep the scan's order
        s, ids = self._finish(s, self._ids_of(best), top_n)
        return (s, ids, (probes, qs, rows, exact)) if return_stages else (s, ids)

    def _file(self, path: str) -> str:
        return self._rank_path(os.path.join(path, _SCANN_FILE))

    def save(self, path: str):
        """scann_index.py:49-50 / dense_retrieval.py:330-336: `path` is a directory (created when missing); this rank's shard
        goes into one numpy .npz archive inside it (`scann_ip.npz`, with `.rank<r>` appended under several ranks)."""
        os.makedirs(path, exist_ok=True)
        self._write_archive(self._file(path), _SCANN_MAGIC, _SCANN_FORMAT, eta=self.eta, centroids=self.centroids,
                            codebook=self.codebook, list_begin=self.list_begin, codes=self.codes, vectors=self.vectors,
                            ids=self.ids)

    def load(self, path: str):
        """scann_index.py:52-53: reads the archive inside the directory.  The file decides what was built (leaves, codebook,
        codes); the config decides how it is searched (leaves to search, reorder)."""
        p = self._file(path)
        if not os.path.isdir(path) or not os.path.exists(p):
            raise ops.NativeError(f"{path} holds no ScannIPIndexer archive ({os.path.basename(p)}): an index serialized by scann "
                                  "cannot be read, build the index again with index()")
        z = self._read_archive(p, "a ScannIPIndexer", _SCANN_MAGIC, _SCANN_FORMAT, "centroids")
        n, nlist = z["vectors"].shape[0], z["centroids"].shape[0]
        lb = z["list_begin"]
        if (z["codes"].shape != (n, self.E_pad // 4) or z["codes"].dtype != np.uint8 or z["vectors"].dtype != np.float16
                or z["ids"].shape != (n,) or z["codebook"].shape != (self.E_pad // 2, 16, 2) or lb.shape != (nlist + 1,)
                or lb[0] != 0 or lb[-1] != n or (np.diff(lb) < 0).any()):
            raise ops.NativeError(f"{p} is damaged: codes {z['codes'].shape} {z['codes'].dtype}, vectors {z['vectors'].shape}, "
                                  f"ids {z['ids'].shape}, codebook {z['codebook'].shape}, list_begin {lb.shape}")
        self.centroids = torch.from_numpy(z["centroids"]).to(self.device)
        self.codebook = torch.from_numpy(z["codebook"]).to(self.device)
        self.list_begin = torch.from_numpy(lb.astype(np.int64)).to(self.device)
        self.codes = torch.from_numpy(z["codes"]).to(self.device)
        self.vectors = torch.from_numpy(z["vectors"]).to(self.device)
        self.ids = torch.from_numpy(z["ids"].astype(np.int64)).to(self.device)
        self.nlist, self.eta = nlist, float(z["eta"])


class MaxPIndexer:
    """Document retrieval over a PASSAGE index (`maxP->bert_dot`, matchmaker/models/max_p_adapter.py:109-151 + the search
    branch dense_retrieval.py:414-429): the inner index holds one vector per passage under its document's id
    (dense_retrieval.py:237-265, `current_ids[start:end] = len(seq_ids)`), a search asks it for `index_hit_top_n` passage
    hits and keeps the first hit of every document until `top_n` documents are found (ops.distinct_hits: one kernel instead
    of the host loop).

    `inner` is any object with `search_device(query_vec, k)`: FlatIPIndexer, IVFFlatIPIndexer, IVFFp8IPIndexer,
    GraphIPIndexer, ScannIPIndexer.  With several ranks the inner search already returns the merged top-k, so a document
    whose passages lie on two shards is deduplicated after the merge.  distinct_fn(scores, ids, top_n) defaults to
    ops.distinct_hits; the CPU test-suite injects a stand-in, as for the other indexers.

    Certificate: the hits are the top-K passages in descending order, so a document with no passage among them scores at
    most the K-th hit, which is at most every listed hit: the kept hits are the document ranking as far as they go.  A query
    is `complete` when its list holds >= top_n documents or fewer than K valid hits (the index ran out); with an exact inner
    index its row is then the exact top_n of all documents.  With an approximate inner index `complete` means that asking
    for more hits cannot add documents the inner search would have found, not that the row is exact."""

    MAX_HITS = ops.DISTINCT_MAX_HITS

    def __init__(self, inner, distinct_fn=None, max_hits: Optional[int] = None):
        """max_hits: where widening stops (default and maximum MAX_HITS, the kernel's limit).  The native inner indexers take
        k <= 4096 (the top-k kernel's candidate sorter): pass max_hits=4096 to widen over one of them."""
        self.inner = inner
        self._distinct = distinct_fn if distinct_fn is not None else ops.distinct_hits
        self.max_hits = self.MAX_HITS if max_hits is None else int(max_hits)
        if not 1 <= self.max_hits <= self.MAX_HITS:
            raise ops.NativeError(f"MaxPIndexer: max_hits={max_hits} outside 1 .. {self.MAX_HITS}", ops._lib.MM_EUNSUPPORTED)

    def prepare(self, *args, **kw):
        return self.inner.prepare(*args, **kw)

    def index(self, ids, data_chunks):
        """As the inner index's: `ids` repeat per passage."""
        return self.inner.index(ids, data_chunks)

    def index_resident(self, ids: torch.Tensor, vectors: torch.Tensor):
        return self.inner.index_resident(ids, vectors)

    def index_store(self, store):
        """The passages of a TokenStore (TokenStoreWriter.finish(): one range of rows per document, the zero rows of the
        [docs, chunks, dim] encoder output already removed) become the inner index: every row under the index of its document
        in store.seq_ids.  The ids are built on the device; the rows are used as they lie when the ranges tile the matrix in
        document order (the writer's layout) and gathered otherwise.  With several ranks each takes its contiguous shard."""
        if store.is_fp8 and store._tokens is None:
            raise ops.NativeError("MaxPIndexer.index_store: an fp8-only store has no 16-bit rows to index; build the passage "
                                  "index with IVFFp8IPIndexer over its codes, or keep the rows (keep_tokens=True)")
        inner, tokens = self.inner, store.tokens
        dev = tokens.device
        begin, end = store._begin, store._end
        length = torch.from_numpy(end - begin).to(dev)
        ids = torch.repeat_interleave(torch.arange(length.numel(), dtype=torch.int64, device=dev), length)
        tiled = begin.size == 0 or (begin[0] == 0 and end[-1] == tokens.shape[0] and bool((begin[1:] == end[:-1]).all()))
        if not tiled:
            first = torch.cumsum(length, 0) - length                        # the document's first row in the packed order
            rows = torch.arange(ids.numel(), dtype=torch.int64, device=dev) + torch.repeat_interleave(
                torch.from_numpy(begin).to(dev) - first, length)
            tokens = tokens[rows]
        world, rank = inner._world() if hasattr(inner, "_world") else (1, 0)
        if world > 1:
            lo, hi = shard_range(ids.numel(), world, rank)
            ids, tokens = ids[lo:hi], tokens[lo:hi]
        vec = tokens.to(inner.device).to(inner.dtype)
        if vec.shape[1] != inner.E_pad:
            if vec.shape[1] > inner.E_pad:
                raise ops.NativeError(f"MaxPIndexer.index_store: {vec.shape[1]}-dim rows for an index of width {inner.E_pad}")
            vec = torch.nn.functional.pad(vec, (0, inner.E_pad - vec.shape[1]))
        inner.index_resident(ids.to(inner.device), vec.contiguous())

    def _check(self, top_n, index_hit_top_n):
        top_n = int(top_n)
        K = int(index_hit_top_n) if index_hit_top_n else top_n      # test_config.get("index_hit_top_n", top_n), dense_retrieval.py:391
        if top_n > self.MAX_HITS or K > self.MAX_HITS:
            raise ops.NativeError(f"MaxPIndexer.search: top_n={top_n} / index_hit_top_n={K} above the limit of {self.MAX_HITS} "
                                  "hits per query (the distinct-hits kernel sorts a query's hits in LDS)", ops._lib.MM_EUNSUPPORTED)
        if not 1 <= top_n <= K:
            raise ops.NativeError(f"MaxPIndexer.search: top_n={top_n} outside 1 .. index_hit_top_n={K}")
        return top_n, K

    def search_device(self, query_vec, top_n: int, index_hit_top_n: Optional[int] = None, widen: bool = False,
                      return_info: bool = False):
        """(scores [nq, top_n] float32, ids [nq, top_n] int64) on the device: the first top_n distinct documents among the
        K = index_hit_top_n (default top_n) passage hits of every query, -inf / -1 where the hits held fewer.
        widen=False: one search and one kernel, no host synchronisation (the reference's behaviour).  widen=True: the
        `complete` flags are read back and the incomplete queries ALONE are searched again with K doubled (capped at
        max_hits) until every query is complete or K is at the cap; rows still incomplete there stay flagged.
        return_info: also a dict of pos [nq, top_n] int32 (the kept hit's position in its list), n_distinct [nq] int32,
        complete [nq] bool and hits_used [nq] int32 (the K of the search the row comes from)."""
        top_n, K = self._check(top_n, index_hit_top_n)
        hs, hi = self.inner.search_device(query_vec, K)
        s, ids, pos, nd, nv = self._distinct(hs, hi, top_n)
        complete = (nd >= top_n) | (nv < K)
        used = torch.full_like(nd, K)
        if widen:
            q = torch.as_tensor(query_vec)
            q = q[None, :] if q.dim() == 1 else q
            while K < self.max_hits:
                todo = torch.nonzero(~complete).flatten()                   # the read-back
                if todo.numel() == 0:
                    break
                K = min(2 * K, self.max_hits)
                hs, hi = self.inner.search_device(q[todo.to(q.device)], K)
                s2, i2, p2, nd2, nv2 = self._distinct(hs, hi, top_n)
                s[todo], ids[todo], pos[todo], nd[todo] = s2, i2, p2, nd2
                complete[todo] = (nd2 >= top_n) | (nv2 < K)
                used[todo] = K
        if return_info:
            return s, ids, {"pos": pos, "n_distinct": nd, "complete": complete, "hits_used": used}
        return s, ids

    def search(self, query_vec, top_n: int, index_hit_top_n: Optional[int] = None, widen: bool = False,
               return_info: bool = False):
        """search_device() as numpy arrays (the info dict's values included)."""
        out = self.search_device(query_vec, top_n, index_hit_top_n, widen, return_info)
        if return_info:
            return out[0].cpu().numpy(), out[1].cpu().numpy(), {k: v.cpu().numpy() for k, v in out[2].items()}
        return out[0].cpu().numpy(), out[1].cpu().numpy()

    def save(self, path: str):
        return self.inner.save(path)

    def load(self, path: str):
        return self.inner.load(path)
