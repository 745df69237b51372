"""A plain restatement of the ranking rule and the metric bodies of matchmaker/utils/core_metrics.py:22-511 on the tensor
form the kernels see (scores, seg_begin, grade, cand_pos) — row by row in Python, independent of matchmaker_amd.metrics'
vectorised numpy route — plus the loaders and the comparison helpers the rank-metrics tests share.

The error bound: AP and nDCG of a query are one division of a sum of m non-negative, correctly rounded float64
terms, summed in possibly different orders on the two sides.  A sum of m such terms in any order is within (m - 1) u of the
exact sum relatively (u = 2^-53, first order), the division adds u on each side:  |got - want| <= 2 (m + 1) u |want|.
The means over nq queries add nq more terms: m_max + nq in place of m.
"""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("edges", "graded", "short1", "short7", "short64")
NOT_JUDGED = -2 ** 31
I32_MAX = 2 ** 31 - 1
U = 2.0 ** -53


def rank_ref(scores, seg_begin):
    """order [N] int32: per segment Python's stable sorted(), higher score first, NaN behind everything."""
    scores = np.asarray(scores, np.float32)
    order = np.zeros(len(scores), np.int32)
    for s in range(len(seg_begin) - 1):
        b, e = int(seg_begin[s]), int(seg_begin[s + 1])
        rows = sorted(range(b, e), key=lambda i: (1, 0.0) if math.isnan(scores[i]) else (0, -float(scores[i])))
        order[b:e] = rows
    return order


def metrics_ref(order, seg_begin, grade, cand_pos, threshold, binp, rcut, ncut, map_cut, bnr, idcg, lg):
    """(first_rank [nq], hits [nq, nR], ap [nq], ndcg [nq, nN], matched [nq]) at one threshold; cand_pos None = plain."""
    nq = len(seg_begin) - 1
    first = np.zeros(nq, np.int32)
    hits = np.zeros((nq, len(rcut)), np.int32)
    ap = np.zeros(nq)
    ndcg = np.zeros((nq, len(ncut)))
    matched = np.zeros(nq, np.int64)
    for q in range(nq):
        rank = k = 0
        any_judged = any_rel = False
        ap_sum, dcg = 0.0, [0.0] * len(ncut)
        for r in range(int(seg_begin[q]), int(seg_begin[q + 1])):
            row = int(order[r])
            g = int(grade[row])
            keep = cand_pos is None or int(cand_pos[row]) <= threshold
            if keep:
                rank += 1
            if g == NOT_JUDGED:
                continue
            matched[q] += 1
            any_judged = True
            rel = g >= binp
            any_rel = any_rel or rel
            if not keep:
                continue
            if rel:
                k += 1
                if first[q] == 0:
                    first[q] = rank
                if rank <= map_cut:
                    ap_sum += k / rank
                for c, cut in enumerate(rcut):
                    hits[q, c] += rank <= cut
            for c, cut in enumerate(ncut):
                if rank <= cut:
                    dcg[c] += g / float(lg[rank])
        if any_rel:
            ap[q] = ap_sum / int(bnr[q])
        if any_judged:
            for c in range(len(ncut)):
                ndcg[q, c] = dcg[c] / idcg[q, c] if idcg[q, c] != 0 else float("nan")      # numpy's 0 / 0
    return first, hits, ap, ndcg, matched


def depth_ref(order, seg_begin, grade, cand_pos, hi, *rest):
    """metrics_ref for t = 1 .. hi, stacked on a new axis 1."""
    per_t = [metrics_ref(order, seg_begin, grade, cand_pos, t, *rest) for t in range(1, hi + 1)]
    return tuple(np.stack([p[i] for p in per_t], axis=1) for i in range(4)) + (per_t[0][4],)


def dict_ref(first, hits, ap, ndcg, bnr, evaluated, rcut, ncut, map_cut):
    """core_metrics.py:464-499 from the per-query quantities."""
    d = {}
    for c, cutoff in enumerate(rcut):
        fr = [int(f) if 0 < f <= cutoff else 0 for f in first]
        rr = [1 / f if f else 0.0 for f in fr]
        nz = [f for f in fr if f]
        d["MRR@" + str(cutoff)] = sum(rr) / evaluated
        d["Recall@" + str(cutoff)] = sum(int(h) / int(b) for h, b in zip(hits[:, c], bnr) if b) / evaluated
        d["QueriesWithNoRelevant@" + str(cutoff)] = len(fr) - len(nz)
        d["QueriesWithRelevant@" + str(cutoff)] = len(nz)
        d["AverageRankGoldLabel@" + str(cutoff)] = float(np.mean(nz)) if nz else 0.0
        d["MedianRankGoldLabel@" + str(cutoff)] = float(np.median(nz)) if nz else 0.0
    for c, cutoff in enumerate(ncut):
        d["nDCG@" + str(cutoff)] = float(np.sum(ndcg[:, c])) / evaluated
    d["QueriesRanked"] = evaluated
    d["MAP@" + str(map_cut)] = float(np.sum(ap)) / evaluated
    return d


# ---- fixtures ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def load_case(name):
    """(json dict, npz arrays) of tests/golden/rank_metrics_<name>.*, read once."""
    if name not in _CACHE:
        with open(os.path.join(GOLDEN, f"rank_metrics_{name}.json")) as f:
            js = json.load(f)
        _CACHE[name] = (js, dict(np.load(os.path.join(GOLDEN, f"rank_metrics_{name}.npz"))))
    return _CACHE[name]


def eval_set(name, **kw):
    from matchmaker_amd.metrics import EvalSet
    js, arr = load_case(name)
    return EvalSet(js["query_ids"], js["doc_ids"], js["qrels"], js["candidate_ranking"], js["binarization_point"], js["config"], **kw)


# ---- comparisons ---------------------------------------------------------------------------------------------------------
EXACT_KEYS = ("QueriesWithNoRelevant@", "QueriesWithRelevant@", "AverageRankGoldLabel@", "MedianRankGoldLabel@", "QueriesRanked")


def assert_close(got, want, m, what=""):
    """|got - want| <= 2 (m + 1) u |want| element-wise (m broadcastable); NaN only where the other side has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN pattern", got, want)
    fin = ~np.isnan(want)
    err = np.abs(np.where(fin, got - want, 0.0))
    bound = 2 * (np.asarray(m) + 1) * U * np.abs(np.where(fin, want, 0.0))
    assert np.all(err <= bound), (what, float(err.max()), got[err > bound][:4], want[err > bound][:4])


def assert_dict(got, want, m_mean, what=""):
    """A metric dict: same keys in the same order; counts, average / median rank and QueriesRanked exactly; the means within
    the bound for m_mean = m_max + nq."""
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        if k.startswith(EXACT_KEYS):
            assert float(got[k]) == float(want[k]), (what, k, got[k], want[k])
        else:
            assert_close(got[k], want[k], m_mean, f"{what} {k}")


def assert_per_query(es, per_query, want_rr, want_ap, want_recall, want_ndcg, matched, what=""):
    """per_query = (first_rank, hits, ap, ndcg) arrays against the reference's return_per_query arrays: RR and recall
    exactly, AP and nDCG within the bound for that query's matched rows."""
    first, hits, ap, ndcg = (np.asarray(x) for x in per_query)
    bnr = es._host["bnr"]
    for c, cutoff in enumerate(es.rcut):
        fr = np.where((first > 0) & (first <= cutoff), first, 0)
        rr = np.array([1 / f if f else 0.0 for f in fr])
        rec = np.array([h / b if b else 0.0 for h, b in zip(hits[:, c], bnr)])
        assert np.array_equal(rr, want_rr[c]), (what, "rr", cutoff)
        assert np.array_equal(rec, want_recall[c]), (what, "recall", cutoff)
    assert_close(ap, want_ap, matched, what + " ap")
    assert_close(ndcg.T, want_ndcg, matched[None, :], what + " ndcg")


def matched_rows(es):
    """Judged rows per query of an EvalSet: the m of the bound."""
    g, sb = es._host["grade"], es._host["seg_begin"]
    return np.array([int((g[sb[q]:sb[q + 1]] != NOT_JUDGED).sum()) for q in range(es.n_queries)], np.int64)
