"""HBM-resident mirror of matchmaker's ColBERT retrieval token store + one-launch aggregation.

The reference writes every document's non-zero token vectors back to back into raw memmaps
`token_reps_<n>.npy` of `token_block_size` rows (matchmaker/dense_retrieval.py:205-206, 246-263),
remembers `doc_infos[seq_id] = (file_no, start, end)` (:265) and `storage_filled_to_index` (:249,
:276), saves them to `doc_infos.npz` (:278-279) and reloads them with np.memmap (:292-303).  Its
ColBERT "aggregate" search step then scores ONE candidate per Python iteration:
`storage[file][start:end] -> torch -> forward_aggregation` (:398-412, colbert.py:100-112).

Here the filled parts of all files live in one device tensor [T, E] (8.8 M MSMARCO passages x ~70
tokens x 128 dims x 2 B = 158 GB fits one MI355X's 288 GB) and a whole batch of
(query, candidate list) pairs is scored by ONE mm_maxsim_ragged_fwd launch that reads the candidate
rows in place (no gather, no padding).

`search` is the whole ColBERT retrieval of :391-412 on the device: token search over the resident matrix
(ops.dot_topk, or an IVFFlatIPIndexer over the token rows), the documents that own the hits
(ops.colbert_candidates), their MaxSim (ops.maxsim_ragged) and the top_n selection (ops.topk_merge).

fp8 mode (opt-in): the store is `codes` [T, E] uint8 (OCP e4m3fn) + `scales` [T] float32 (one power of two per
row) instead of the 16-bit matrix — half the resident bytes (158 GB -> 81 GB for MS MARCO at dim 128) and half the bytes the
MaxSim stage streams.  `quantize_fp8()`, `from_reference_parts(..., fp8=True)`, `load(..., fp8=True)` and `load_fp8()` build
one; aggregate / rank_hits / search_device / search then score through ops.maxsim_ragged_fp8.  The token search runs on the
codes themselves with `token_search="fp8"` (ops.dot_topk_fp8): an fp8-ONLY store then retrieves end to end and
the memory figure holds for the whole of search().  `build_token_index(config)` gives the IVF alternative to that brute-force
search: for an fp8 store an IVFFp8IPIndexer whose lists are codes + scales as well (ops.ivf_scan_fp8), passed as
`index=`.  Without either the token search needs 16-bit rows, as before: an `index=` that holds 16-bit vectors of its own, or
the rows kept with `keep_tokens=True`.
`row_shard=` runs a flat token search (16-bit or fp8) over consecutive shards of that many rows and merges the per-shard
lists (ops.topk_merge): the one-call search places its sampled threshold only up to about 1.3 M rows at k' = 128
(DESIGN §3.12); `row_shard = 2**20` is the recommended setting for stores beyond that.

`TokenStoreWriter` builds a store on the device straight from encoder output: `append(seq_ids, vecs)` per batch
(ops.store_append: the zero-row removal and doc_infos of dense_retrieval.py:232-265 as a stream compaction, 16-bit rows and / or
fp8 codes + scales), `finish()` for the TokenStore; `TokenStore.save_reference` writes a store back in the reference's layout.
"""
import glob
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


class TokenStore:
    def __init__(self, tokens: Optional[torch.Tensor], seq_ids: Sequence, begin: np.ndarray, end: np.ndarray,
                 topk_fn=None, candidates_fn=None, maxsim_fn=None, merge_fn=None, *, codes: Optional[torch.Tensor] = None,
                 scales: Optional[torch.Tensor] = None, source_dtype: Optional[torch.dtype] = None, quantize_fn=None,
                 topk_fp8_fn=None):
        """topk_fn(queries, matrix, k) / candidates_fn(hit_rows, begin_sorted, end_sorted, doc_of_sorted, T, c_cap) /
        maxsim_fn(q, tokens, begin, end, None, pairs_per_query=, check_ranges=, sim_round=) / merge_fn(scores, ids, k) are what
        search() runs; they default to ops.dot_topk / ops.colbert_candidates / ops.maxsim_ragged / ops.topk_merge (the CPU
        test-suite injects stand-ins, as for the indexers of retrieval.py).
        fp8 mode: codes [T, E] uint8 + scales [T] float32 (ops.fp8_quantize_rows' format) make the store an fp8 one; `tokens`
        may then be None (the 16-bit rows are not resident) or the rows kept for the token search.  maxsim_fn is then called as
        maxsim_fn(q, codes, scales, begin, end, None, pairs_per_query=, check_ranges=, sim_round=) and defaults to
        ops.maxsim_ragged_fp8; source_dtype is the dtype the rows were quantised from (it picks the query's 16-bit type);
        quantize_fn(x) -> (codes, scales) is what quantize_fp8() and the fp8 loaders run (default ops.fp8_quantize_rows);
        topk_fp8_fn(q16, codes, scales, k) is the token search of token_search="fp8" (default ops.dot_topk_fp8)."""
        self._fp8 = codes is not None
        if self._fp8:
            if scales is None or codes.dim() != 2 or codes.dtype != torch.uint8 or tuple(scales.shape) != (codes.shape[0],):
                raise ops.NativeError("TokenStore: an fp8 store is codes [T, E] uint8 + scales [T] float32")
            if tokens is not None and (tokens.shape != codes.shape or tokens.device != codes.device):
                raise ops.NativeError("TokenStore: the kept token rows and the fp8 codes differ in shape or device")
        elif tokens is None:
            raise ops.NativeError("TokenStore: needs the token matrix, or codes + scales of an fp8 store")
        self._topk = topk_fn if topk_fn is not None else ops.dot_topk
        self._candidates = candidates_fn if candidates_fn is not None else ops.colbert_candidates
        self._maxsim = maxsim_fn if maxsim_fn is not None else (ops.maxsim_ragged_fp8 if self._fp8 else ops.maxsim_ragged)
        self._merge = merge_fn if merge_fn is not None else ops.topk_merge
        self._quantize = quantize_fn if quantize_fn is not None else ops.fp8_quantize_rows
        self._topk_fp8 = topk_fp8_fn if topk_fp8_fn is not None else ops.dot_topk_fp8
        self._tokens = tokens                         # [T, E] on the scoring device (read-only: the ranges below were validated against it)
        self._tokens_lowp = None                      # fp16 image of an fp32 store, built on the first use_fp16 aggregate()
        self._codes, self._scales = codes, scales
        self._device = codes.device if self._fp8 else tokens.device
        self._n_rows = int(codes.shape[0] if self._fp8 else tokens.shape[0])
        self._source_dtype = source_dtype if source_dtype is not None else (tokens.dtype if tokens is not None else torch.float16)
        self.seq_ids = list(seq_ids)
        self._index = {s: i for i, s in enumerate(self.seq_ids)}
        self._begin = np.asarray(begin, dtype=np.int64)   # global row ranges per document
        self._end = np.asarray(end, dtype=np.int64)
        # validated once, on the host copy of doc_infos: the scoring calls then skip the per-call device check
        if self._begin.size and (self._begin.min() < 0 or self._end.max() > self._n_rows or (self._begin > self._end).any()):
            raise ops.NativeError(f"TokenStore: document ranges leave the {self._n_rows}-row token matrix "
                                  "(doc_infos of another store?)")
        self._build_sorted_view()

    def _build_sorted_view(self):
        """The documents that hold rows, sorted by (begin, end): what search() finds the owner of a token row in.
        Zero-length documents own no row and are left out; gaps between documents are allowed; two non-empty ranges that
        overlap are refused, because a row of the overlap would have two owners."""
        keep = np.nonzero(self._end > self._begin)[0]
        order = keep[np.lexsort((self._end[keep], self._begin[keep]))]
        b, e = self._begin[order], self._end[order]
        clash = np.nonzero(b[1:] < e[:-1])[0]
        if clash.size:
            i, j = int(order[clash[0]]), int(order[clash[0] + 1])
            raise ops.NativeError(f"TokenStore: documents {self.seq_ids[i]!r} (rows {self._begin[i]}..{self._end[i]}) and "
                                  f"{self.seq_ids[j]!r} (rows {self._begin[j]}..{self._end[j]}) overlap: a token row must "
                                  "belong to one document")
        if len(self.seq_ids) >= 2 ** 31:
            raise ops.NativeError("TokenStore: more than 2^31-1 documents")
        dev = self._device
        self._begin_sorted = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
        self._end_sorted = torch.from_numpy(np.ascontiguousarray(e)).to(dev)
        self._doc_of_sorted = torch.from_numpy(order.astype(np.int32)).to(dev)

    @property
    def tokens(self) -> torch.Tensor:
        """The resident token matrix.  Read-only: aggregate() skips the per-call range check because the document ranges
        were validated against THIS matrix in the constructor — build a new TokenStore for another matrix."""
        if self._tokens is None:
            raise ops.NativeError("TokenStore.tokens: this is an fp8 store built without keep_tokens=True — the 16-bit rows are "
                                  "not resident; read .codes / .scales (ops.fp8_dequantize_rows gives their values)")
        return self._tokens

    @property
    def is_fp8(self) -> bool:
        return self._fp8

    @property
    def codes(self) -> torch.Tensor:
        """[T, E] uint8, OCP e4m3fn bytes of an fp8 store (read-only, like .tokens)."""
        if not self._fp8:
            raise ops.NativeError("TokenStore.codes: not an fp8 store (quantize_fp8() makes one)")
        return self._codes

    @property
    def scales(self) -> torch.Tensor:
        """[T] float32, the power-of-two row scales of an fp8 store."""
        if not self._fp8:
            raise ops.NativeError("TokenStore.scales: not an fp8 store (quantize_fp8() makes one)")
        return self._scales

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_reference_parts(cls, storage: List[np.ndarray], doc_infos: Dict, seq_ids: Sequence, device, fp8: bool = False,
                             **fns):
        """storage[n] = filled part of token_reps_<n>.npy; doc_infos / seq_ids as saved by the
        reference (dense_retrieval.py:265-266, 278-279).  fp8=True: every file is quantised as it arrives and only its codes
        and scales are kept — the 16-bit matrix is never resident as a whole.  fns: the constructor's *_fn arguments."""
        base = np.concatenate([[0], np.cumsum([s.shape[0] for s in storage])]).astype(np.int64)
        begin = np.empty(len(seq_ids), dtype=np.int64)
        end = np.empty(len(seq_ids), dtype=np.int64)
        for i, sid in enumerate(seq_ids):
            f, a, b = doc_infos[sid]
            begin[i], end[i] = base[f] + a, base[f] + b
        E = storage[0].shape[1]
        T = int(base[-1])
        if fp8:
            quantize = fns.get("quantize_fn") or ops.fp8_quantize_rows
            codes = torch.empty((T, E), dtype=torch.uint8, device=device)
            scales = torch.empty((T,), dtype=torch.float32, device=device)
            src = torch.from_numpy(np.empty(0, dtype=storage[0].dtype)).dtype
            for n, part in enumerate(storage):        # file by file: one file's 16-bit rows at a time
                c, s = quantize(torch.from_numpy(np.array(part)).to(device))
                codes[int(base[n]): int(base[n + 1])] = c
                scales[int(base[n]): int(base[n + 1])] = s
            return cls(None, seq_ids, begin, end, codes=codes, scales=scales, source_dtype=src, **fns)
        tokens = torch.empty((T, E), dtype=torch.from_numpy(np.empty(0, dtype=storage[0].dtype)).dtype, device=device)
        for n, part in enumerate(storage):            # file by file: no second host copy of the store
            tokens[int(base[n]): int(base[n + 1])] = torch.from_numpy(np.array(part)).to(device)
        return cls(tokens, seq_ids, begin, end, **fns)

    @classmethod
    def load(cls, folder: str, token_dim: int, token_dtype: str, token_block_size: int, device, fp8: bool = False, **fns):
        """Reads a folder written by `dense_retrieval.py encode` (same calls as :292-303).  fp8=True: quantised file by
        file into an fp8 store (from_reference_parts)."""
        dfs = np.load(os.path.join(folder, "doc_infos.npz"), allow_pickle=True)
        doc_infos = dfs.get("doc_infos")[()]
        seq_ids = dfs.get("seq_ids")[()]
        filled = dfs.get("storage_filled_to_index")[()]
        storage = []
        for f in range(len(glob.glob(os.path.join(folder, "token_reps_*")))):
            mm = np.memmap(os.path.join(folder, "token_reps_" + str(f) + ".npy"), dtype=np.dtype(token_dtype),
                           mode="r", shape=(token_block_size, token_dim))
            storage.append(mm[: int(filled[f])])
        return cls.from_reference_parts(storage, doc_infos, list(seq_ids), device, fp8=fp8, **fns)

    def quantize_fp8(self, keep_tokens: bool = False, maxsim_fn=None) -> "TokenStore":
        """The fp8 store of this one: same documents, rows as e4m3fn codes + one power-of-two scale each
        (ops.fp8_quantize_rows; per element |value - x| <= 2^-4 |x| + 2^-10 scale).  keep_tokens=True keeps a reference to
        the 16-bit rows for token_hits() without index= (no memory is saved then, only MaxSim bytes).  maxsim_fn: the fp8
        store's scoring function (default ops.maxsim_ragged_fp8); the other injected functions carry over."""
        if self._fp8:
            raise ops.NativeError("TokenStore.quantize_fp8: already an fp8 store")
        codes, scales = self._quantize(self._tokens)
        return TokenStore(self._tokens if keep_tokens else None, self.seq_ids, self._begin, self._end, topk_fn=self._topk,
                          candidates_fn=self._candidates, maxsim_fn=maxsim_fn, merge_fn=self._merge, codes=codes, scales=scales,
                          source_dtype=self._tokens.dtype, quantize_fn=self._quantize, topk_fp8_fn=self._topk_fp8)

    def save_fp8(self, folder: str) -> None:
        """Writes an fp8 store with numpy: codes.npy [T, E] uint8, scales.npy [T] float32 and docs.npz (seq_ids, begin, end,
        source_dtype).  The format is this project's own; the reference has no quantised store."""
        if not self._fp8:
            raise ops.NativeError("TokenStore.save_fp8: not an fp8 store (quantize_fp8() makes one)")
        os.makedirs(folder, exist_ok=True)
        np.save(os.path.join(folder, "codes.npy"), self._codes.cpu().numpy())
        np.save(os.path.join(folder, "scales.npy"), self._scales.cpu().numpy())
        ids = np.empty(len(self.seq_ids), dtype=object)
        ids[:] = list(self.seq_ids)
        np.savez(os.path.join(folder, "docs.npz"), seq_ids=ids, begin=self._begin, end=self._end,
                 source_dtype=np.array(str(self._source_dtype).replace("torch.", "")))

    def save_reference(self, folder: str, token_block_size: int, token_dtype: Optional[str] = None) -> None:
        """Writes a 16-bit or fp32 store in the reference's layout (dense_retrieval.py:205-206, 246-279): raw memmaps
        `token_reps_<n>.npy` of token_block_size rows, the documents in seq_ids order, no document straddling a file, and
        `doc_infos.npz` — byte for byte what write_reference_store writes for the same documents, so the reference's
        skip-encoding branch (:291-302) and TokenStore.load read it.  token_dtype: numpy's name of the files' dtype (default:
        the store's own; the rows are cast with torch when it differs).  Runs of documents that are neighbours in the store
        and in a file cross to the host in one copy."""
        if self._tokens is None:
            raise ops.NativeError("TokenStore.save_reference: an fp8-only store holds no rows the reference's layout can take — "
                              "save_fp8() writes it")
        name = token_dtype or str(self._tokens.dtype).replace("torch.", "")
        if name not in ("float16", "float32"):
            raise ops.NativeError(f"TokenStore.save_reference: token_dtype={name!r}: numpy memmaps hold float16 or float32 (pass one)")
        np_dt, t_dt = np.dtype(name), getattr(torch, name)
        token_block_size = int(token_block_size)
        lens = self._end - self._begin
        if lens.size and int(lens.max()) > token_block_size:
            raise ops.NativeError(f"TokenStore.save_reference: a document of {int(lens.max())} rows does not fit a file of "
                              f"token_block_size={token_block_size}")
        os.makedirs(folder, exist_ok=True)
        E = int(self._tokens.shape[1])

        def new_file(n):
            return np.memmap(os.path.join(folder, f"token_reps_{n}.npy"), dtype=np_dt, mode="w+", shape=(token_block_size, E))

        n, ins = 0, 0
        base = new_file(0)
        doc_infos, filled = {}, []
        run = None                                       # [store row from, store row to, file row]: one pending copy

        def flush_run():
            if run is not None:
                a, b, at = run
                base[at: at + (b - a)] = self._tokens[a:b].to(t_dt).cpu().numpy()

        for i, sid in enumerate(self.seq_ids):
            k, a = int(lens[i]), int(self._begin[i])
            if ins + k > token_block_size:               # :248-256 start the next file
                flush_run()
                run = None
                filled.append(ins)
                base.flush()
                n, ins = n + 1, 0
                base = new_file(n)
            if k:
                if run is not None and run[1] == a:
                    run[1] = a + k
                else:
                    flush_run()
                    run = [a, a + k, ins]
            doc_infos[sid] = (n, ins, ins + k)
            ins += k
        flush_run()
        filled.append(ins)
        base.flush()
        ids = np.empty(len(self.seq_ids), dtype=object)
        ids[:] = list(self.seq_ids)
        np.savez(os.path.join(folder, "doc_infos.npz"), doc_infos=np.array(doc_infos, dtype=object), seq_ids=ids,
                 storage_filled_to_index=np.array(filled), id_mapping=np.array([], dtype=object))

    @classmethod
    def load_fp8(cls, folder: str, device, **fns) -> "TokenStore":
        """Reads a folder written by save_fp8 onto `device`.  fns: the constructor's *_fn arguments."""
        docs = np.load(os.path.join(folder, "docs.npz"), allow_pickle=True)
        codes = torch.from_numpy(np.load(os.path.join(folder, "codes.npy"))).to(device)
        scales = torch.from_numpy(np.load(os.path.join(folder, "scales.npy"))).to(device)
        src = getattr(torch, str(docs["source_dtype"][()]))
        return cls(None, list(docs["seq_ids"]), docs["begin"], docs["end"], codes=codes, scales=scales, source_dtype=src, **fns)

    # ------------------------------------------------------------------ lookup + scoring
    def ranges(self, seq_ids: Iterable) -> Tuple[torch.Tensor, torch.Tensor]:
        idx = np.fromiter((self._index[s] for s in seq_ids), dtype=np.int64)
        dev = self._device
        return torch.from_numpy(self._begin[idx]).to(dev), torch.from_numpy(self._end[idx]).to(dev)

    def aggregate(self, query_vecs: torch.Tensor, candidates: Sequence[Sequence],
                  use_fp16: bool = True) -> List[List[Tuple[object, float]]]:
        """query_vecs [nq, Q, E] (forward_representation output, already multiplied by its mask as in
        `search_type="encode"`); candidates[i] = the seq_ids to re-score for query i (the set the
        reference loops over, :400-402).  use_fp16: the searcher head's autocast switch (indexing_heads.py:49-56,
        `model_config["use_fp16"]` at :407): the stored rows go through `.float()` and autocast's cast back — the same fp16
        values — and `bmm` / `max` return fp16, so every per-token maximum is rounded to fp16 before the fp32 sum;
        False = fp32 similarities of the stored values.  An fp32 store (`token_dtype: float32`) under use_fp16 is scored as
        the reference's autocast scores it: `bmm` casts BOTH operands to fp16 first, so the store's fp16 image (built once, on
        the first such call: +50 % of the store's memory) and the fp16 query are what the kernel reads — MM_SIM_ROUND alone
        would be a no-op on fp32 rows.  An fp8 store is scored by ops.maxsim_ragged_fp8: use_fp16=True = an fp16 query and
        every per-token maximum rounded to fp16; False = the query in the 16-bit type the rows were quantised from (bf16 for
        an fp32 source) and fp32 through max and sum.  Returns, per query, [(seq_id, score)] like
        `validation_results[query_id]` (:410)."""
        nq = query_vecs.shape[0]
        if len(candidates) != nq:
            raise ValueError(f"{nq} queries but {len(candidates)} candidate lists")
        counts = [len(c) for c in candidates]
        C = max(counts) if counts else 0
        if C == 0:
            return [[] for _ in range(nq)]
        # one launch: pad every list to C pairs with empty ranges (an empty range costs nothing)
        flat, pad = [], []
        for c in candidates:
            flat.extend(c)
            pad.append(C - len(c))
        b, e = self.ranges(flat)
        bb = torch.zeros((nq, C), dtype=torch.int64, device=b.device)
        ee = torch.zeros((nq, C), dtype=torch.int64, device=b.device)
        off = 0
        for i, n in enumerate(counts):
            bb[i, :n], ee[i, :n] = b[off: off + n], e[off: off + n]
            off += n
        if self._fp8:
            scores = self._maxsim(query_vecs.to(self._device).to(self._fp8_query_dtype(use_fp16)), self._codes, self._scales,
                                  bb.view(-1), ee.view(-1), None, pairs_per_query=C, check_ranges=False,
                                  sim_round=bool(use_fp16)).view(nq, C)
        else:
            tokens = self._scoring_tokens(use_fp16)
            q = query_vecs.to(tokens.dtype)
            scores = ops.maxsim_ragged(q, tokens, bb.view(-1), ee.view(-1), None, pairs_per_query=C, check_ranges=False,
                                       sim_round=bool(use_fp16)).view(nq, C)
        scores = scores.cpu()
        return [[(candidates[i][j], float(scores[i, j])) for j in range(counts[i])] for i in range(nq)]

    def _scoring_tokens(self, use_fp16: bool) -> torch.Tensor:
        """The matrix the MaxSim reads: the store, or the fp16 image of an fp32 store under use_fp16 (see aggregate())."""
        tokens = self.tokens
        if use_fp16 and tokens.dtype == torch.float32:
            if self._tokens_lowp is None:
                self._tokens_lowp = tokens.to(torch.float16)
            tokens = self._tokens_lowp
        return tokens

    def _fp8_query_dtype(self, use_fp16: bool) -> torch.dtype:
        """The 16-bit type of the query an fp8 store is scored with (see aggregate())."""
        if use_fp16:
            return torch.float16
        return self._source_dtype if self._source_dtype in (torch.float16, torch.bfloat16) else torch.bfloat16

    # ------------------------------------------------------------------ retrieval: query token vectors -> ranked documents
    def build_token_index(self, config, subsample=-1, native_kmeans: bool = True, **fns):
        """An IVF index over the token rows, for token_hits(index=) / search_device(index=): its ids are token rows.
        config: the indexer's keys (faiss_ivf_list_count, faiss_ivf_search_probe_count, optionally random_seed); token_dim is
        the store's width.  An fp8 store gets an IVFFp8IPIndexer trained on a seeded sample of the rows
        dequantised to float16 (train_codes) and filled with index_codes(arange(T), codes, scales): the lists are a
        list-ordered copy of codes + scales, no 16-bit row is ever resident.  A 16-bit store gets an IVFFlatIPIndexer trained
        and filled with the float16 rows (train_resident / index_resident).  subsample in (0, 1) trains on that fraction of
        the rows; fns: the indexer's *_fn arguments (the CPU test-suite injects stand-ins)."""
        from .retrieval import IVFFlatIPIndexer, IVFFp8IPIndexer, _pad_dim
        E = int(self._codes.shape[1] if self._fp8 else self._tokens.shape[1])
        if _pad_dim(E) != E:
            raise ops.NativeError(f"TokenStore.build_token_index: the store's width {E} is not one of 128, 256, 384, 512, 768 "
                                  "(pad the rows)", ops._lib.MM_EUNSUPPORTED)
        cfg = dict(config)
        cfg["token_dim"] = E
        ids = torch.arange(self._n_rows, dtype=torch.int64, device=self._device)
        if self._fp8:
            ix = IVFFp8IPIndexer(cfg, device=self._device, native_kmeans=native_kmeans, **fns)
            ix.train_codes(self._codes, self._scales, subsample=subsample)
            ix.index_codes(ids, self._codes, self._scales)
        else:
            fns.pop("quantize_fn", None)                 # (the 16-bit lists quantise nothing)
            ix = IVFFlatIPIndexer(cfg, device=self._device, native_kmeans=native_kmeans, **fns)
            rows = self._scoring_tokens(True)
            rows = rows if rows.dtype == torch.float16 else rows.to(torch.float16)
            ix.train_resident(rows, subsample=subsample)
            ix.index_resident(ids, rows)
        return ix

    def token_hits(self, query_vecs: torch.Tensor, token_top_k: int, index=None,
                   query_chunk: Optional[int] = None, token_search: Optional[str] = None,
                   row_shard: Optional[int] = None) -> torch.Tensor:
        """Steps 1-3 of search_device: hit_rows [nq, Q * token_top_k] int64 = for every LIVE query token (a vector with a
        non-zero element; `search_type="encode"` multiplies by the mask, so padding is zero rows) the exact token_top_k rows of
        the store by inner product of the 16-bit values (ops.dot_topk: equal scores go to the lower row), -1 for dead tokens.
        index: an indexer whose ids are token rows — what build_token_index() returns (an IVFFp8IPIndexer over codes + scales
        for an fp8 store, an IVFFlatIPIndexer for a 16-bit one), or an IVFFlatIPIndexer built by hand with
        index_resident(ids=arange(T), vectors=tokens); its probed lists are then searched instead of the whole matrix.
        query_chunk bounds the tokens per search call.
        token_search="fp8" (an fp8 store only, not together with index=): the search runs over codes + scales
        (ops.dot_topk_fp8; the query in the 16-bit type of the rows the store was quantised from, fp16 for an fp32 source), so an
        fp8-only store needs neither index= nor keep_tokens=True.  None: the 16-bit search as before — an fp8 store then
        needs index= (build_token_index() makes one that holds fp8 lists), or the rows kept by keep_tokens=True.
        row_shard (a positive multiple of 64; the flat searches only, not with index=): the rows are searched in consecutive
        shards of row_shard rows and a running [n, k] list is merged with each shard's result (ops.topk_merge, the running
        list first: equal scores still go to the lower row).  None: one call.  2**20 is the recommended shard for stores
        beyond the one-call envelope of DESIGN §3.12."""
        nq, Q, E = query_vecs.shape
        k = int(token_top_k)
        if k < 1 or Q * k > ops.COLBERT_MAX_HITS:
            raise ops.NativeError(f"TokenStore.search: Q * token_top_k = {Q} * {k} hits per query outside 1 .. "
                                  f"{ops.COLBERT_MAX_HITS} (the candidate kernel sorts a query's hits in 64 KB of LDS)",
                                  ops._lib.MM_EUNSUPPORTED)
        if token_search is not None:
            if token_search != "fp8":
                raise ops.NativeError(f"TokenStore.token_hits: token_search={token_search!r} (None or \"fp8\")")
            if not self._fp8:
                raise ops.NativeError("TokenStore.token_hits: token_search=\"fp8\" needs an fp8 store (quantize_fp8() makes one)")
            if index is not None:
                raise ops.NativeError("TokenStore.token_hits: token_search= and index= are two searches — pass one")
        if row_shard is not None:
            if index is not None:
                raise ops.NativeError("TokenStore.token_hits: row_shard= shards the flat search — not with index=")
            if int(row_shard) != row_shard or row_shard <= 0 or row_shard % 64:
                raise ops.NativeError(f"TokenStore.token_hits: row_shard={row_shard!r} must be a positive multiple of 64")
        fp8_search = token_search == "fp8"
        if self._tokens is None and index is None and not fp8_search:
            raise ops.NativeError("TokenStore.token_hits: an fp8 store holds no 16-bit rows to search — pass index= (an "
                                  "indexer over the token rows; build_token_index() makes an fp8 one) or build the store "
                                  "with keep_tokens=True (or search the codes themselves: token_search=\"fp8\")",
                                  ops._lib.MM_EUNSUPPORTED)
        dev = self._device
        q = query_vecs.to(dev).reshape(nq * Q, E)
        live = torch.nonzero((q != 0).any(dim=1)).flatten()
        hits = torch.full((nq * Q, k), -1, dtype=torch.int64, device=dev)
        if self._tokens is None or fp8_search:           # fp8 store + index / fp8 search: the dtype the 16-bit matrix would have had
            matrix = None
            qs = q.to(self._source_dtype if self._source_dtype != torch.float32 else torch.float16)
        else:
            matrix = self._scoring_tokens(True)          # the 16-bit matrix: the store, or an fp32 store's fp16 image
            qs = q.to(matrix.dtype)
        step = int(query_chunk) if query_chunk else max(int(live.numel()), 1)
        for a in range(0, int(live.numel()), step):
            sel = live[a: a + step]
            if index is not None:
                rows = index.search_device(qs[sel], k)[1]
            else:
                rows = self._flat_search(qs[sel].contiguous(), matrix, k, fp8_search, row_shard)
            hits[sel] = rows
        return hits.view(nq, Q * k)

    def _flat_search(self, q16: torch.Tensor, matrix: Optional[torch.Tensor], k: int, fp8_search: bool,
                     row_shard: Optional[int]) -> torch.Tensor:
        """rows [n, k] of the flat token search: over codes + scales (fp8_search) or the 16-bit matrix, in one call or in
        consecutive shards of row_shard rows merged into a running list (see token_hits())."""
        def one(lo, hi):
            if fp8_search:
                return self._topk_fp8(q16, self._codes[lo:hi], self._scales[lo:hi], k)
            return self._topk(q16, matrix[lo:hi], k)
        T = self._n_rows
        if row_shard is None or row_shard >= T:
            return one(0, T)[1]
        run_s = run_i = None
        for lo in range(0, T, int(row_shard)):
            s, i = one(lo, min(lo + int(row_shard), T))
            i = torch.where(i >= 0, i + lo, i)           # -1 (a shard shorter than k) stays -1
            if run_s is None:
                run_s, run_i = s, i
            else:                                        # the running list first: input order on ties = lower row first
                run_s, run_i = self._merge(torch.cat([run_s, s], dim=1), torch.cat([run_i, i], dim=1), k)
        return run_i

    def rank_hits(self, query_vecs: torch.Tensor, hit_rows: torch.Tensor, top_n: int, use_fp16: bool = True,
                  trim: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """Steps 4-7 of search_device: the documents that own hit_rows [nq, H], their MaxSim against query_vecs, the top_n.
        trim=False keeps min(H, documents) candidate slots per query instead of reading the largest count back: nothing
        then synchronises and the four launches can be captured into a graph (one chain, no parallel branches)."""
        nq = query_vecs.shape[0]
        dev = self._device
        n_docs = int(self._begin_sorted.numel())
        if nq == 0 or n_docs == 0:
            return (torch.full((nq, top_n), float("-inf"), dtype=torch.float32, device=dev),
                    torch.full((nq, top_n), -1, dtype=torch.int64, device=dev))
        cand_doc, cb, ce, count = self._candidates(hit_rows, self._begin_sorted, self._end_sorted, self._doc_of_sorted,
                                                   self._n_rows, min(hit_rows.shape[1], n_docs))
        if trim:
            C = max(int(count.max()), 1)                 # the one read-back: the slots behind it are padding in every query
            cand_doc, cb, ce = cand_doc[:, :C].contiguous(), cb[:, :C].contiguous(), ce[:, :C].contiguous()
        C = cand_doc.shape[1]
        if self._fp8:
            scores = self._maxsim(query_vecs.to(dev).to(self._fp8_query_dtype(use_fp16)), self._codes, self._scales,
                                  cb.view(-1), ce.view(-1), None, pairs_per_query=C, check_ranges=False,
                                  sim_round=bool(use_fp16)).view(nq, C)
        else:
            tokens = self._scoring_tokens(use_fp16)
            scores = self._maxsim(query_vecs.to(dev).to(tokens.dtype), tokens, cb.view(-1), ce.view(-1), None, pairs_per_query=C,
                                  check_ranges=False, sim_round=bool(use_fp16)).view(nq, C)
        scores = scores.masked_fill(cand_doc < 0, float("-inf"))
        # ascending cand_doc + the merge's input order on ties = equal scores go to the lower document index
        return self._merge(scores, cand_doc.to(torch.int64), int(top_n))

    def search_device(self, query_vecs: torch.Tensor, top_n: int, token_top_k: int, use_fp16: bool = True, index=None,
                      query_chunk: Optional[int] = None, trim: bool = True, token_search: Optional[str] = None,
                      row_shard: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """ColBERT retrieval (dense_retrieval.py:391-412) for query_vecs [nq, Q, E], without a host round trip per query:
          1-3. token_hits(): the token_top_k best token rows of every live query token (token_search / row_shard as there:
               token_search="fp8" makes the whole retrieval run on an fp8-only store);
          4.   the candidates = the documents that own at least one hit row (ops.colbert_candidates);
          5.   one read-back of the largest candidate count, to trim the slots (trim=False: none, see rank_hits());
          6.   forward_aggregation of the query against every candidate, exactly as aggregate() computes it (use_fp16 as
               there; dead query tokens add 0);
          7.   the top_n by score, equal scores to the lower document index.
        Returns (scores [nq, top_n] float32 descending, doc_idx [nq, top_n] int64 = positions in self.seq_ids); (-inf, -1)
        where a query has fewer than top_n candidates."""
        hits = self.token_hits(query_vecs, token_top_k, index=index, query_chunk=query_chunk, token_search=token_search,
                               row_shard=row_shard)
        return self.rank_hits(query_vecs, hits, top_n, use_fp16=use_fp16, trim=trim)

    def search(self, query_vecs: torch.Tensor, top_n: int, token_top_k: int, use_fp16: bool = True, index=None,
               query_chunk: Optional[int] = None, token_search: Optional[str] = None,
               row_shard: Optional[int] = None) -> List[List[Tuple[object, float]]]:
        """search_device() mapped to the reference's result shape: per query [(seq_id, score)] best first, like
        `validation_results[query_id]` (:410-412); shorter than top_n when the query has fewer candidates."""
        s, d = self.search_device(query_vecs, top_n, token_top_k, use_fp16=use_fp16, index=index, query_chunk=query_chunk,
                                  token_search=token_search, row_shard=row_shard)
        s, d = s.cpu().numpy(), d.cpu().numpy()
        ids = self.seq_ids
        return [[(ids[j], float(x)) for x, j in zip(s[i], d[i]) if j >= 0] for i in range(s.shape[0])]


class TokenStoreWriter:
    """Builds a TokenStore on the device from encoder output, batch by batch: the host half of the reference's encode loop
    (dense_retrieval.py:232-265 — the copy of the padded batch to the CPU, the per-document removal of zero rows, the copy
    into a memmap, doc_infos) as one native call per batch (ops.store_append).

        w = TokenStoreWriter(capacity_rows, token_dim, dtype=torch.float16, device="cuda", fp8=False)
        w.append(seq_ids, vecs)        # vecs [B, D, E]: all-zero rows are padding and dropped; [B, E]: one row each, all kept
        store = w.finish()             # -> TokenStore

    The writer owns the store's buffers — rows [capacity_rows, token_dim] of `dtype`, or codes + scales with fp8=True, or both
    with keep_tokens=True — a growing device table of the documents' row ranges, and the device-side fill / status the
    appends chain through.  append() does not synchronise while the running sum of B * D stays within the capacity; see there.
    append_fn: what append() runs (default ops.store_append; the CPU test-suite injects a stand-in, as for the indexers);
    fns: TokenStore's *_fn arguments, handed to the store finish() builds."""

    def __init__(self, capacity_rows: int, token_dim: int, dtype: torch.dtype = torch.float16, device="cuda", fp8: bool = False,
                 keep_tokens: bool = False, append_fn=None, **fns):
        if dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise ops.NativeError(f"TokenStoreWriter: dtype {dtype} (float16, bfloat16 or float32)")
        self.capacity, self.token_dim, self.dtype = int(capacity_rows), int(token_dim), dtype
        if self.capacity < 0 or self.token_dim < 1:
            raise ops.NativeError(f"TokenStoreWriter: capacity_rows={capacity_rows}, token_dim={token_dim}")
        self._device = torch.device(device)
        self._fp8 = bool(fp8)
        self._append = append_fn if append_fn is not None else ops.store_append
        self._fns = fns
        dev, T, E = self._device, self.capacity, self.token_dim
        self._tokens = torch.empty((T, E), dtype=dtype, device=dev) if (not fp8 or keep_tokens) else None
        self._codes = torch.empty((T, E), dtype=torch.uint8, device=dev) if fp8 else None
        self._scales = torch.empty((T,), dtype=torch.float32, device=dev) if fp8 else None
        self._fill = torch.zeros(1, dtype=torch.int64, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._table = torch.full((2, 1024), -1, dtype=torch.int64, device=dev)   # begin / end per document; -1 = never written
        self.seq_ids: List = []
        self._seen = set()
        self.rows_upper_bound = 0                        # >= the device-side fill, without reading it
        self._finished = False

    def _grow_table(self, n: int):
        cap = self._table.shape[1]
        if n <= cap:
            return
        while cap < n:
            cap *= 2
        table = torch.full((2, cap), -1, dtype=torch.int64, device=self._device)
        table[:, : len(self.seq_ids)] = self._table[:, : len(self.seq_ids)]
        self._table = table

    def append(self, seq_ids: Sequence, vecs: torch.Tensor) -> None:
        """vecs [B, D, E]: document i's token rows, all-zero rows being padding (the model multiplies by its mask,
        colbert.py:95-96) — they are dropped, wherever in the document they are.  vecs [B, E]: one vector per document, kept
        even if zero (the reference's dim_count == 1 case).  Rows are converted to the store's dtype.
        Nothing synchronises while rows_upper_bound (the running sum of B * D) stays within the capacity.  When it would pass
        it, the device-side fill is read back once and takes the bound's place; if even that true fill cannot take B * D more
        rows, NativeError is raised before anything is launched.  Otherwise the batch is launched and the device decides: a
        batch that does not fit writes nothing and sets the sticky status finish() reports."""
        if self._finished:
            raise ops.NativeError("TokenStoreWriter.append: finish() was called — the buffers belong to the store now")
        seq_ids = list(seq_ids)
        keep_all = vecs.dim() == 2
        if keep_all:
            vecs = vecs.unsqueeze(1)
        if vecs.dim() != 3 or vecs.shape[0] != len(seq_ids) or vecs.shape[2] != self.token_dim:
            raise ops.NativeError(f"TokenStoreWriter.append: {len(seq_ids)} seq_ids and vectors {tuple(vecs.shape)}: expected "
                                  f"[B, D, {self.token_dim}] or [B, {self.token_dim}]")
        new = set()
        for s in seq_ids:
            if s in self._seen or s in new:
                raise ops.NativeError(f"TokenStoreWriter.append: seq_id {s!r} was appended before")
            new.add(s)
        B, D = int(vecs.shape[0]), int(vecs.shape[1])
        if B == 0:
            return
        n = B * D
        if self.rows_upper_bound + n > self.capacity:
            true = int(self._fill.item())                # the one read-back
            if true + n > self.capacity:
                raise ops.NativeError(f"TokenStoreWriter.append: the store holds {true} of {self.capacity} rows and cannot take a "
                                      f"batch of {B} x {D} = {n} rows (document {seq_ids[0]!r} on)", ops._lib.MM_EUNSUPPORTED)
            self.rows_upper_bound = true
        vecs = vecs.to(self._device)
        # the kernel converts fp32 <-> 16-bit on the way; an fp8 store is quantised from the values of the store's dtype, as
        # from_reference_parts(fp8=True) quantises the stored rows
        if vecs.dtype != self.dtype and (self._fp8 or torch.float32 not in (vecs.dtype, self.dtype)):
            vecs = vecs.to(self.dtype)
        n0 = len(self.seq_ids)
        self._grow_table(n0 + B)
        self._append(vecs, self._tokens, self._codes, self._scales, self.capacity, self._fill, self._table[0, n0: n0 + B],
                     self._table[1, n0: n0 + B], self._status, keep_zero_rows=keep_all)
        self.rows_upper_bound += n
        self.seq_ids.extend(seq_ids)
        self._seen |= new

    def finish(self, compact: bool = False) -> "TokenStore":
        """Reads fill, status and the document table back (once each) and returns the TokenStore over the filled part of the
        buffers — views; compact=True clones them to their exact size, so the unused capacity can be freed.  Raises
        NativeError naming the first document that did not fit when an append was refused on the device."""
        fill, status = int(self._fill.item()), int(self._status.item())
        n = len(self.seq_ids)
        table = self._table[:, :n].cpu().numpy()
        if status != 0:
            first = int(np.argmax(table[0] < 0)) if n else 0
            raise ops.NativeError(f"TokenStoreWriter.finish: the store's {self.capacity} rows were full at {fill}: the batch of "
                                  f"document {self.seq_ids[first]!r} (number {first}) did not fit and nothing after it was "
                                  "written — build a writer with a larger capacity_rows", ops._lib.MM_EUNSUPPORTED)
        self._finished = True
        cut = (lambda t: None if t is None else (t[:fill].clone() if compact else t[:fill]))
        tokens, codes, scales = cut(self._tokens), cut(self._codes), cut(self._scales)
        self._tokens = self._codes = self._scales = None
        if self._fp8:
            return TokenStore(tokens, self.seq_ids, table[0], table[1], codes=codes, scales=scales, source_dtype=self.dtype,
                              **self._fns)
        return TokenStore(tokens, self.seq_ids, table[0], table[1], **self._fns)


def write_reference_store(folder: str, docs: Sequence[np.ndarray], seq_ids: Sequence, token_block_size: int,
                          token_dtype: str = "float16"):
    """Writes `docs` (each [n_tokens, E]) exactly as dense_retrieval.py:205-279 lays them out (raw
    memmap blocks + doc_infos.npz in numpy's npz container, :278 saveCompressed = stored zip of .npy).
    Used by the tests and for building synthetic stores; the reference's own writer is its encode loop."""
    os.makedirs(folder, exist_ok=True)
    E = docs[0].shape[1]
    n, ins = 0, 0
    base = np.memmap(os.path.join(folder, f"token_reps_{n}.npy"), dtype=np.dtype(token_dtype), mode="w+",
                     shape=(token_block_size, E))
    doc_infos, filled = {}, []
    for sid, reps in zip(seq_ids, docs):
        reps = reps[np.abs(reps).sum(-1) > 0, :]                         # :244 zero rows are padding
        k = reps.shape[0]
        if ins + k > token_block_size:                                   # :248-256 start the next file
            filled.append(ins)
            base.flush()
            n, ins = n + 1, 0
            base = np.memmap(os.path.join(folder, f"token_reps_{n}.npy"), dtype=np.dtype(token_dtype), mode="w+",
                             shape=(token_block_size, E))
        base[ins: ins + k] = reps
        doc_infos[sid] = (n, ins, ins + k)
        ins += k
    filled.append(ins)
    base.flush()
    ids = np.empty(len(seq_ids), dtype=object)
    ids[:] = list(seq_ids)
    np.savez(os.path.join(folder, "doc_infos.npz"), doc_infos=np.array(doc_infos, dtype=object), seq_ids=ids,
             storage_filled_to_index=np.array(filled), id_mapping=np.array([], dtype=object))
