"""Ranking and IR metrics from scores that stay on the device (matchmaker/utils/core_metrics.py:22-511).

The reference's evaluation step takes `{query_id: [(doc_id, score), ...]}`, sorts every query with Python's `sorted`
(:502-511) and walks the ranked id lists with numpy, query by query (:22-499).  Here the string ids are joined ONCE, on the
host, into flat per-row tensors (`EvalSet`); a validation pass then hands over nothing but its scores:

    es = EvalSet(query_ids, doc_ids, qrels, candidate_ranking).to("cuda")       # once per candidate file
    metrics = es.metrics_plain(scores)                                          # scores [N], arrival order, any device

HIP tensors take the kernels of rank_metrics.hip (ops.segment_rank / rank_metrics / rank_metrics_depth); CPU tensors, a
segment longer than ops.RANK_MAX_LEN, or `native=False` take the numpy route of this module, which computes the same
per-query quantities from the same tensors.  Both end in the same host code that builds the reference's dict.

Stated choices where the reference leaves the result undefined or fails:
  * NaN scores rank after everything else (-inf included), in arrival order;
  * zero evaluated queries (no ranked query is in the qrels) raises ValueError — the reference divides by zero;
  * negative or non-integer grades, and a judged query whose candidate ranking is missing (or lacks one of its documents),
    are refused when the EvalSet is built — the reference raises KeyError in the middle of the pass for the latter.
"""
import copy
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# utils/core_metrics.py:12-16
global_metric_config = {
    "MRR+Recall@": [10, 20, 100, 200, 1000],
    "nDCG@": [3, 5, 10, 20, 1000],
    "MAP@": 1000,
}

NOT_JUDGED = -2 ** 31             # ops.RANK_NOT_JUDGED
_I32_MAX = 2 ** 31 - 1
DEPTH_OUTPUT_BUDGET = 256 << 20   # bytes of per-(query, threshold) outputs one sweep launch may produce (query_chunk=None)


# ---- the numpy route: the same per-query quantities from the same flat arrays ------------------------------------------
def np_segment_rank(scores: np.ndarray, seg_begin: np.ndarray) -> np.ndarray:
    """order [N] int32 of ops.segment_rank: one stable lexicographic sort by (segment, NaN last, score descending)."""
    scores = np.asarray(scores, dtype=np.float32)
    n = scores.shape[0]
    seg = np.repeat(np.arange(len(seg_begin) - 1), np.diff(seg_begin))
    nan = np.isnan(scores)
    neg = np.where(nan, np.float32(0), -scores)
    return np.lexsort((neg, nan, seg)).astype(np.int32) if n else np.zeros(0, np.int32)


def _np_query(cp, g, thresholds, binp, rcut, ncut, map_cut, bnr, idcg, lg):
    """One query: cp / g [len] in rank order (cp None: nothing is dropped), thresholds [T].  Only judged rows matter, so the
    merged rank of each of them is counted per threshold: (first_rank [T], hits [T, nR], ap [T], ndcg [T, nN])."""
    T = len(thresholds)
    first = np.zeros(T, np.int32)
    hits = np.zeros((T, len(rcut)), np.int32)
    ap = np.zeros(T)
    ndcg = np.zeros((T, len(ncut)))
    pos = np.nonzero(g != NOT_JUDGED)[0]
    if pos.size == 0:
        return first, hits, ap, ndcg
    gm = g[pos].astype(np.float64)
    if cp is None:
        adm = np.ones((T, pos.size), bool)
        rank = np.broadcast_to(pos + 1, (T, pos.size))
    else:
        adm = cp[pos][None, :] <= thresholds[:, None]
        # merged rank of judged row j at threshold t = rows i <= pos[j] with cp[i] <= t
        top = min(int(thresholds.max()), int(cp.max()))
        rank = np.empty((T, pos.size), np.int64)
        for j, p in enumerate(pos):
            below = np.cumsum(np.bincount(np.clip(cp[:p + 1], 0, top + 1), minlength=top + 2))
            rank[:, j] = below[np.clip(thresholds, 0, top + 1)]
    rel = gm >= binp
    if rel.any():
        ra = adm & rel[None, :]
        k = np.cumsum(ra, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(ra & (rank <= map_cut), k / rank, 0.0)
        ap = term.sum(axis=1) / bnr
        for c, cut in enumerate(rcut):
            hits[:, c] = (ra & (rank <= cut)).sum(axis=1)
        has = ra.any(axis=1)
        first = np.where(has, np.where(ra, rank, _I32_MAX).min(axis=1), 0).astype(np.int32)
    for c, cut in enumerate(ncut):
        on = adm & (rank <= cut)
        with np.errstate(divide="ignore", invalid="ignore"):
            dcg = np.where(on, gm[None, :] / lg[np.where(on, rank, 0)], 0.0).sum(axis=1)
            ndcg[:, c] = dcg / idcg[c]
    return first, hits, ap, ndcg


def np_rank_metrics(order, seg_begin, grade, cand_pos, thresholds, binp, rcut, ncut, map_cut, bnr, idcg, lg):
    """ops.rank_metrics_depth's outputs for an arbitrary list of thresholds: ([nq, T], [nq, T, nR], [nq, T], [nq, T, nN])."""
    nq, T = len(seg_begin) - 1, len(thresholds)
    thresholds = np.asarray(thresholds, np.int64)
    first = np.zeros((nq, T), np.int32)
    hits = np.zeros((nq, T, len(rcut)), np.int32)
    ap = np.zeros((nq, T))
    ndcg = np.zeros((nq, T, len(ncut)))
    for q in range(nq):
        rows = order[seg_begin[q]:seg_begin[q + 1]]
        first[q], hits[q], ap[q], ndcg[q] = _np_query(None if cand_pos is None else cand_pos[rows], grade[rows], thresholds, binp,
                                                      rcut, ncut, map_cut, bnr[q], idcg[q], lg)
    return first, hits, ap, ndcg


# ---- per-query quantities -> the reference's dict -----------------------------------------------------------------------
def _rr_and_rank(first_rank: np.ndarray, cutoff: int):
    fr = np.where((first_rank > 0) & (first_rank <= cutoff), first_rank, 0)
    with np.errstate(divide="ignore"):
        rr = np.where(fr > 0, 1.0 / np.maximum(fr, 1), 0.0)
    return rr, fr


def _nonzero_stat(fr: np.ndarray, fn):
    """fn (nanmean / nanmedian) of the non-zero ranks along the query axis, 0 where there is none (:468-472)."""
    import warnings
    v = np.where(fr > 0, fr.astype(np.float64), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        out = fn(v, axis=0)
    return np.nan_to_num(out, nan=0.0)


class EvalSet:
    """The host-side join of one candidate file with the qrels, reusable across validations.

    query_ids / doc_ids [N]: the (query, document) pairs in ARRIVAL order — the order the scores will come in.  Queries are
    numbered in first-arrival order, which is the key order of the reference's `ranking` dict; the rows of a query are its
    segment, in arrival order (they need not arrive next to each other).
    qrels {qid: {did: grade}} (load_qrels); candidate_ranking {qid: {did: 1-based first-stage rank}} or None.
    cutoffs: a dict like global_metric_config (at most 8 MRR+Recall and 8 nDCG cutoffs)."""

    def __init__(self, query_ids: Sequence, doc_ids: Sequence, qrels: Dict, candidate_ranking: Optional[Dict] = None,
                 binarization_point: float = 1.0, cutoffs: Optional[Dict] = None):
        if len(query_ids) != len(doc_ids):
            raise ValueError(f"EvalSet: {len(query_ids)} query ids for {len(doc_ids)} doc ids")
        cfg = dict(global_metric_config if cutoffs is None else cutoffs)
        self.rcut = [int(c) for c in cfg["MRR+Recall@"]]
        self.ncut = [int(c) for c in cfg["nDCG@"]]
        self.map_cut = int(cfg["MAP@"])
        if len(self.rcut) > 8 or len(self.ncut) > 8 or min(self.rcut + self.ncut + [self.map_cut]) < 1:
            raise ValueError("EvalSet: at most 8 MRR+Recall@ and 8 nDCG@ cutoffs, each >= 1")
        self.binarization_point = float(binarization_point)
        n = len(query_ids)
        qindex: Dict = {}
        qi = np.empty(n, np.int64)
        for i, qid in enumerate(query_ids):
            qi[i] = qindex.setdefault(qid, len(qindex))
        self.qids = list(qindex)
        nq = len(self.qids)
        perm = np.argsort(qi, kind="stable")                    # segment-major row -> arrival row
        self._identity = bool(np.array_equal(perm, np.arange(n)))
        counts = np.bincount(qi, minlength=nq) if n else np.zeros(nq, np.int64)
        seg_begin = np.zeros(nq + 1, np.int64)
        np.cumsum(counts, out=seg_begin[1:])
        self.docs = [doc_ids[i] for i in perm]                 # segment-major, arrival order inside a segment
        self.arrival_ids = (list(query_ids), list(doc_ids))    # what a caller's batches are checked against
        self.max_len = int(counts.max()) if nq else 0
        grade = np.full(n, NOT_JUDGED, np.int32)
        cand = None if candidate_ranking is None else np.full(n, _I32_MAX, np.int32)
        in_qrels = np.zeros(nq, bool)
        bnr = np.zeros(nq, np.int32)
        idcg = np.ones((nq, len(self.ncut)))
        for q, qid in enumerate(self.qids):
            if qid not in qrels:                                # :381 — ranked, not evaluated: its rows stay unjudged
                continue
            in_qrels[q] = True
            judged = qrels[qid]
            grades = np.array(list(judged.values()), dtype=np.float64)
            if grades.size and (grades.min() < 0 or np.any(grades != np.floor(grades)) or grades.max() >= _I32_MAX):
                raise ValueError(f"EvalSet: query {qid!r} has a negative or non-integer grade (grades are int32 on the device)")
            bnr[q] = int((grades >= self.binarization_point).sum())
            srt = np.sort(grades)[::-1]
            for c, cut in enumerate(self.ncut):                 # :447, the reference's own expression
                idcg[q, c] = (srt[:cut] / np.log2(1 + np.arange(1, min(grades.size, cut) + 1))).sum()
            b, e = int(seg_begin[q]), int(seg_begin[q + 1])
            for r in range(b, e):
                g = judged.get(self.docs[r])
                if g is not None:
                    grade[r] = int(g)
            if cand is not None:
                if qid not in candidate_ranking:
                    raise ValueError(f"EvalSet: query {qid!r} is judged but has no candidate ranking")
                cq = candidate_ranking[qid]
                for r in range(b, e):
                    p = cq.get(self.docs[r])
                    if p is None:
                        raise ValueError(f"EvalSet: document {self.docs[r]!r} of query {qid!r} is not in its candidate ranking")
                    cand[r] = int(p)
        self.evaluated_queries = int(in_qrels.sum())
        self.in_qrels = in_qrels
        lg = np.log2(1 + np.arange(0, max(self.ncut + [1]) + 2))
        self.t = {"perm": torch.from_numpy(perm), "seg_begin": torch.from_numpy(seg_begin), "grade": torch.from_numpy(grade),
                  "bnr": torch.from_numpy(bnr), "idcg": torch.from_numpy(idcg), "log2": torch.from_numpy(lg)}
        if cand is not None:
            self.t["cand_pos"] = torch.from_numpy(cand)
        self._host = {k: v.numpy() for k, v in self.t.items()}

    # ---- plumbing ----
    @property
    def device(self):
        return self.t["grade"].device

    @property
    def n_rows(self) -> int:
        return self.t["grade"].shape[0]

    @property
    def n_queries(self) -> int:
        return len(self.qids)

    def to(self, device) -> "EvalSet":
        """A view of this set whose tensors live on `device` (the host copies and the id lists are shared)."""
        other = copy.copy(self)
        other.t = {k: v.to(device) for k, v in self.t.items()}
        return other

    def _native(self, scores: torch.Tensor, native: Optional[bool], bound: int) -> bool:
        from . import ops
        if native is False or not scores.is_cuda:
            if native and not scores.is_cuda:
                raise ops.NativeError("EvalSet: native=True needs HIP device scores")
            return False
        if bound > ops.RANK_MAX_LEN:
            if native:
                raise ops.NativeError(f"EvalSet: {bound} rows per segment / thresholds above the native limit of "
                                      f"{ops.RANK_MAX_LEN}", ops._lib.MM_EUNSUPPORTED)
            return False
        if self.device != scores.device:
            raise ops.NativeError(f"EvalSet on {self.device}, scores on {scores.device}: move the set with .to(device) once")
        return True

    def _segment_major(self, scores: torch.Tensor) -> torch.Tensor:
        if scores.dim() != 1 or scores.shape[0] != self.n_rows:
            raise ValueError(f"EvalSet: expected {self.n_rows} scores, got {tuple(scores.shape)}")
        if self._identity:
            return scores
        return scores[self.t["perm"].to(scores.device)]

    # ---- ranking ----
    def rank(self, scores: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
        """order [N] int32 on the scores' device: order[seg_begin[s] + r] = the row (of this set: segment-major) with rank
        r + 1 in query s."""
        s = self._segment_major(scores)
        if self._native(scores, native, self.max_len):
            from . import ops
            return ops.segment_rank(s, self.t["seg_begin"], self.max_len)
        sc = s.detach().float().cpu().numpy()
        return torch.from_numpy(np_segment_rank(sc, self._host["seg_begin"])).to(scores.device)

    def ranked_result(self, scores: torch.Tensor, native: Optional[bool] = None, order: Optional[torch.Tensor] = None) -> Dict:
        """The reference's `{query_id: [doc ids, best first]}` (unrolled_to_ranked_result, :502-511)."""
        order = (self.rank(scores, native) if order is None else order).cpu().numpy()
        sb = self._host["seg_begin"]
        return {qid: [self.docs[r] for r in order[sb[q]:sb[q + 1]]] for q, qid in enumerate(self.qids)}

    # ---- per-query quantities ----
    def per_query(self, scores: torch.Tensor, threshold: Optional[int] = None, native: Optional[bool] = None,
                  order: Optional[torch.Tensor] = None):
        """(first_rank [nq], hits [nq, nR], ap [nq], ndcg [nq, nN]) on the scores' device, nothing read back on the native
        route (graph-capturable).  threshold None: the plain form."""
        if threshold is not None and "cand_pos" not in self.t:
            raise ValueError("EvalSet: a candidate threshold needs candidate_ranking")
        use = self._native(scores, native, self.max_len)
        if order is None:
            order = self.rank(scores, native)
        if use:
            from . import ops
            return ops.rank_metrics(order, self.t["seg_begin"], self.t["grade"], None if threshold is None else self.t["cand_pos"],
                                    _I32_MAX if threshold is None else int(threshold), self.binarization_point, self.rcut,
                                    self.ncut, self.map_cut, self.t["bnr"], self.t["idcg"], self.t["log2"])
        h = self._host
        out = np_rank_metrics(order.cpu().numpy(), h["seg_begin"], h["grade"], None if threshold is None else h["cand_pos"],
                              [_I32_MAX if threshold is None else int(threshold)], self.binarization_point, self.rcut, self.ncut,
                              self.map_cut, h["bnr"], h["idcg"], h["log2"])
        return tuple(torch.from_numpy(np.ascontiguousarray(a[:, 0])).to(scores.device) for a in out)

    def _need_evaluated(self):
        if self.evaluated_queries == 0:
            raise ValueError("EvalSet: none of the ranked queries is in the qrels (the reference divides by zero here)")

    def metrics_from_per_query(self, first_rank, hits, ap, ndcg, return_per_query: bool = False):
        """The reference's dict (:464-499) from per_query's four arrays (tensors or numpy arrays)."""
        self._need_evaluated()
        first_rank, hits, ap, ndcg = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                                      for x in (first_rank, hits, ap, ndcg))
        ev = self.evaluated_queries
        bnr = self._host["bnr"].astype(np.float64)
        d: Dict = {}
        rr_all, rec_all = [], []
        for c, cutoff in enumerate(self.rcut):
            rr, fr = _rr_and_rank(first_rank, cutoff)
            rec = np.where(bnr > 0, hits[:, c] / np.maximum(bnr, 1), 0.0)
            rr_all.append(rr)
            rec_all.append(rec)
            d["MRR@" + str(cutoff)] = rr.sum() / ev
            d["Recall@" + str(cutoff)] = rec.sum() / ev
            d["QueriesWithNoRelevant@" + str(cutoff)] = (rr == 0).sum()
            d["QueriesWithRelevant@" + str(cutoff)] = (rr > 0).sum()
            d["AverageRankGoldLabel@" + str(cutoff)] = _nonzero_stat(fr, np.nanmean)[()]
            d["MedianRankGoldLabel@" + str(cutoff)] = _nonzero_stat(fr, np.nanmedian)[()]
        for c, cutoff in enumerate(self.ncut):
            d["nDCG@" + str(cutoff)] = ndcg[:, c].sum() / ev
        d["QueriesRanked"] = ev
        d["MAP@" + str(self.map_cut)] = ap.sum() / ev
        if return_per_query:
            nq = self.n_queries
            return (d, np.array(rr_all).reshape(len(self.rcut), nq), ap, np.array(rec_all).reshape(len(self.rcut), nq),
                    np.ascontiguousarray(ndcg.T))
        return d

    # ---- the reference's three entry points ----
    def metrics_plain(self, scores, return_per_query: bool = False, native: Optional[bool] = None):
        """calculate_metrics_plain(ranked_result(scores), qrels, binarization_point, return_per_query) (:365-499)."""
        self._need_evaluated()
        return self.metrics_from_per_query(*self.per_query(scores, None, native), return_per_query=return_per_query)

    def metrics_single_candidate_threshold(self, scores, candidate_threshold: int, return_per_query: bool = False,
                                           native: Optional[bool] = None):
        """calculate_metrics_single_candidate_threshold(...) (:212-363)."""
        self._need_evaluated()
        return self.metrics_from_per_query(*self.per_query(scores, int(candidate_threshold), native),
                                           return_per_query=return_per_query)

    def metrics_along_candidate_depth(self, scores, candidate_range: Tuple[int, int], native: Optional[bool] = None,
                                      query_chunk: Optional[int] = None, order: Optional[torch.Tensor] = None) -> Dict[int, Dict]:
        """calculate_metrics_along_candidate_depth(...) (:22-210): {t: dict} for t = lo .. hi.
        query_chunk: queries per sweep launch (None: as many as keep a launch's outputs under DEPTH_OUTPUT_BUDGET bytes).
        first_rank is kept whole for the medians; the float64 sums are accumulated chunk by chunk."""
        lo, hi = int(candidate_range[0]), int(candidate_range[1])
        if "cand_pos" not in self.t:
            raise ValueError("EvalSet: the candidate-depth sweep needs candidate_ranking")
        if hi < 1 or lo < 1 or lo > hi:
            raise ValueError(f"EvalSet: candidate_range {candidate_range!r} needs 1 <= lo <= hi")
        if self.max_len > hi:                                   # the reference's broadcast error (:88-92), before any launch
            raise ValueError(f"EvalSet: a query has {self.max_len} ranked documents, more than candidate_range[1] = {hi}")
        self._need_evaluated()
        nq, nR, nN = self.n_queries, len(self.rcut), len(self.ncut)
        use = self._native(scores, native, max(hi, self.max_len))
        if order is None:
            order = self.rank(scores, native)
        per = hi * (4 + 4 * nR + 8 + 8 * nN)
        chunk = max(1, int(query_chunk) if query_chunk is not None else DEPTH_OUTPUT_BUDGET // per)
        first = np.zeros((nq, hi), np.int32)
        rec_sum, ap_sum, ndcg_sum = np.zeros((hi, nR)), np.zeros(hi), np.zeros((hi, nN))
        h = self._host
        sb = h["seg_begin"]
        for q0 in range(0, nq, chunk):
            q1 = min(nq, q0 + chunk)
            b, e = int(sb[q0]), int(sb[q1])
            if use:
                from . import ops
                t = self.t
                fr, hits, ap, ndcg = ops.rank_metrics_depth(order[b:e] - b, t["seg_begin"][q0:q1 + 1] - b, t["grade"][b:e],
                                                            t["cand_pos"][b:e], hi, self.binarization_point, self.rcut, self.ncut,
                                                            self.map_cut, t["bnr"][q0:q1], t["idcg"][q0:q1], t["log2"])
                bn = t["bnr"][q0:q1].to(torch.float64).clamp(min=1)[:, None, None]
                rec_sum += (hits.to(torch.float64) / bn).sum(0).cpu().numpy()
                ap_sum += ap.sum(0).cpu().numpy()
                ndcg_sum += ndcg.sum(0).cpu().numpy()
                first[q0:q1] = fr.cpu().numpy()
            else:
                o = order.cpu().numpy() if isinstance(order, torch.Tensor) else order
                fr, hits, ap, ndcg = np_rank_metrics(o[b:e] - b, sb[q0:q1 + 1] - b, h["grade"][b:e], h["cand_pos"][b:e],
                                                     np.arange(1, hi + 1), self.binarization_point, self.rcut, self.ncut,
                                                     self.map_cut, h["bnr"][q0:q1], h["idcg"][q0:q1], h["log2"])
                rec_sum += (hits / np.maximum(h["bnr"][q0:q1], 1).astype(np.float64)[:, None, None]).sum(0)
                ap_sum += ap.sum(0)
                ndcg_sum += ndcg.sum(0)
                first[q0:q1] = fr
        ev = self.evaluated_queries
        cols = {}
        for c, cutoff in enumerate(self.rcut):
            rr, fr = _rr_and_rank(first, cutoff)
            cols[cutoff] = (rr.sum(0) / ev, rec_sum[:, c] / ev, (rr == 0).sum(0), (rr > 0).sum(0), _nonzero_stat(fr, np.nanmean),
                            _nonzero_stat(fr, np.nanmedian))
        ndcg_mean, map_mean = ndcg_sum / ev, ap_sum / ev
        result = {}
        for t in range(lo, hi + 1):
            d = {}
            for cutoff in self.rcut:
                mrr, rec, non, relv, avg, med = cols[cutoff]
                d["MRR@" + str(cutoff)] = mrr[t - 1]
                d["Recall@" + str(cutoff)] = rec[t - 1]
                d["QueriesWithNoRelevant@" + str(cutoff)] = non[t - 1]
                d["QueriesWithRelevant@" + str(cutoff)] = relv[t - 1]
                d["AverageRankGoldLabel@" + str(cutoff)] = avg[t - 1]
                d["MedianRankGoldLabel@" + str(cutoff)] = med[t - 1]
            for c, cutoff in enumerate(self.ncut):
                d["nDCG@" + str(cutoff)] = ndcg_mean[t - 1, c]
            d["QueriesRanked"] = ev
            d["MAP@" + str(self.map_cut)] = map_mean[t - 1]
            result[t] = d
        return result
